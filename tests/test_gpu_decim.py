"""Acquisition resampler on the device (gsdr_decim_*, csrc/decim.hip): GNU Radio's
fir_filter_ccf with decimation d between two device rings,

    y[m] = sum_j t[j] x[m*d - j]   over absolute sample indices, x = 0 before the
                                    source's first pushed sample,

against an fp64 restatement; byte-identical output however the input was pushed;
windows through the output ring's mirror; acquisition in place on the decimated
ring; the reference's GPS capture decimated 4 -> 2 Msps; error returns."""
import ctypes
import functools

import numpy as np
import pytest

import gsdr
from gsdr import synth

from conftest import vnorm_rel

pytestmark = pytest.mark.gpu

NIN = 60000
BASE = 1237  # first_sample of the source ring: no multiple of any d below
CHUNKS = (1, 7, 4096, 333, 10, 2500)
SRC_CAP, SRC_WIN = 1 << 15, 1 << 14
OUT_CAP, OUT_WIN = 4096, 2048
ITEMS = {"gr_complex": gsdr.ITEM_GR_COMPLEX, "cshort": gsdr.ITEM_CSHORT, "ibyte": gsdr.ITEM_IBYTE}
CASES = [(2, 9), (8, 39), (10, 49), (3, 7)]


def designed_taps(d):
    """The flowgraph's design for decimation d (gnss_flowgraph.cc:1073-1087) at a 2 Msps output."""
    fs = 2e6 * d
    return gsdr.firdes_low_pass(1.0, fs, 2e6 / 2.1, 2e6 / 2.0)


@functools.lru_cache(maxsize=None)
def taps_of(d, T):
    if (d, T) == (3, 7):
        # arbitrary and asymmetric: a reversed tap order fails
        return np.array([0.9, -0.35, 0.2, 0.11, -0.07, 0.045, 0.3], np.float32)
    t = designed_taps(d)
    assert len(t) == T
    return t


@functools.lru_cache(maxsize=None)
def source_items(item):
    """(items as pushed, the same samples as complex128): unit-variance noise, integers for the integer types."""
    rng = np.random.default_rng(20261019 + ITEMS[item])
    if item == "gr_complex":
        x = (rng.standard_normal(NIN) + 1j * rng.standard_normal(NIN)).astype(np.complex64) * np.float32(np.sqrt(0.5))
        return x, x.astype(np.complex128)
    scale, lim, dt = (1000.0, 32767, np.int16) if item == "cshort" else (20.0, 127, np.int8)
    q = np.clip(np.rint(rng.standard_normal(2 * NIN) * scale * np.sqrt(0.5)), -lim, lim).astype(dt)
    return q, q[0::2].astype(np.float64) + 1j * q[1::2].astype(np.float64)


def fir_decim_ref(x, taps, d, base):
    """fp64 restatement: (m0, y[m0 .. m1)) with zero history before `base`."""
    c = np.convolve(np.asarray(x, np.complex128), np.asarray(taps, np.float64))  # c[k] = sum_j t[j] x[base + k - j]
    m0 = -(-base // d)
    m1 = (base + len(x) - 1) // d + 1
    k = np.arange(m0, m1) * d - base
    return m0, c[k]


@functools.lru_cache(maxsize=None)
def reference(item, d, T):
    return fir_decim_ref(source_items(item)[1], taps_of(d, T), d, BASE)


def chunk_schedule():
    done, k, out = 0, 0, []
    while done < NIN:
        n = min(CHUNKS[k % len(CHUNKS)], NIN - done)
        out.append(n)
        done += n
        k += 1
    return out


def run_schedule(item, d, T, chunks, advance_every=1, src_cap=SRC_CAP, out_cap=OUT_CAP, out_win=OUT_WIN):
    """Push the source in `chunks`, advance after every advance_every-th push (and
    after the last), read each new stretch of the output ring before it is overwritten.
    -> (first output index, outputs, the decimated ring's final head, source head)."""
    items, _ = source_items(item)
    per = 1 if item == "gr_complex" else 2
    src = gsdr.Stream(ITEMS[item], src_cap, SRC_WIN)
    dec = gsdr.Decimator(src, d, taps_of(d, T), out_cap, out_win)
    got, first, read_to, pos = [], None, None, 0
    try:
        for i, n in enumerate(chunks):
            src.push(items[pos * per:(pos + n) * per], BASE + pos)
            pos += n
            if (i + 1) % advance_every and i + 1 < len(chunks):
                continue
            head = dec.advance()
            if first is None:
                if head == 0:
                    continue  # no output ready yet
                # the first output index: ceil(BASE / d) is in the ring, the index before it is not
                first = read_to = -(-BASE // d)
                with pytest.raises(gsdr.GsdrError):
                    dec.output.read(first - 1, 1)
            assert head - read_to <= out_cap
            if head > read_to:
                got.append(dec.output.read(read_to, head - read_to))
                read_to = head
        return first, np.concatenate(got), read_to, BASE + pos
    finally:
        dec.close()
        src.close()


@pytest.mark.parametrize("item", list(ITEMS))
@pytest.mark.parametrize("d,T", CASES)
def test_parity_with_fp64_restatement(item, d, T):
    """A. Measured on MI355X: see DESIGN.md (acquisition resampler); an fp32 chain of
    <= 49 fused multiply-adds sits near 1e-7 relative."""
    m0, ref = reference(item, d, T)
    first, y, head, head_src = run_schedule(item, d, T, chunk_schedule())
    assert first == m0 == -(-BASE // d)
    assert head == (head_src - 1) // d + 1
    assert len(y) == len(ref) == head - m0
    rel = vnorm_rel(y, ref)
    worst = float(np.max(np.abs(y.astype(np.complex128) - ref)))
    print("decim parity %s d=%d T=%d: vnorm_rel %.3e, max|err| %.3e of max|y| %.3e" % (
        item, d, T, rel, worst, float(np.max(np.abs(ref)))))
    assert rel <= 1e-4
    assert worst <= 1e-4 * float(np.max(np.abs(ref)))


@pytest.mark.parametrize("item", list(ITEMS))
@pytest.mark.parametrize("d,T", CASES)
def test_chunking_invariance(item, d, T):
    """B. One push and one advance (several kernel passes over a larger source ring),
    the chunked schedule, and the chunked schedule advanced every fifth push give the
    same bytes."""
    chunks = chunk_schedule()
    f1, y1, h1, _ = run_schedule(item, d, T, [NIN], src_cap=1 << 16, out_cap=1 << 15, out_win=OUT_WIN)
    f2, y2, h2, _ = run_schedule(item, d, T, chunks)
    f3, y3, h3, _ = run_schedule(item, d, T, chunks, advance_every=5)
    assert f1 == f2 == f3 and h1 == h2 == h3
    assert y1.tobytes() == y2.tobytes()
    assert y1.tobytes() == y3.tobytes()


def _device_bytes(ptr, nbytes):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_window_through_the_mirror():
    """C. A window of the output ring that straddles `cap` is one contiguous device span."""
    d, T, item = 2, 9, "gr_complex"
    m0, ref = reference(item, d, T)
    items, _ = source_items(item)
    src = gsdr.Stream(ITEMS[item], SRC_CAP, SRC_WIN)
    dec = gsdr.Decimator(src, d, taps_of(d, T), OUT_CAP, OUT_WIN)
    try:
        # outputs up to index cap + 1000, in pushes the output ring can hold
        need = (OUT_CAP + 1000) * d - BASE
        pos = 0
        while pos < need:
            n = min(4000, need - pos)
            src.push(items[pos:pos + n], BASE + pos)
            pos += n
            head = dec.advance()
        assert head == OUT_CAP + 1000
        first, n = OUT_CAP - 1000, 2000
        ptr = dec.output.window(first, n)
        flat = _device_bytes(ptr, 8 * n).view(np.complex64)
        want = ref[first - m0:first - m0 + n]
        np.testing.assert_array_equal(flat, dec.output.read(first, n))
        assert vnorm_rel(flat, want) <= 1e-4
        assert float(np.max(np.abs(flat - want))) <= 1e-4 * float(np.max(np.abs(want)))
        # the longest window ending at the head is contiguous too
        f, k = dec.output.span()
        assert f + k == head and k == OUT_WIN
        np.testing.assert_array_equal(_device_bytes(dec.output.window(f, k), 8 * k).view(np.complex64),
                                      dec.output.read(f, k))
    finally:
        dec.close()
        src.close()


def test_acquisition_on_the_decimated_ring():
    """D. run_stream on the decimator's output equals run on the same decimated items from the host."""
    fs, d, N, nblk = 4000000, 2, 2000, 3
    sats = synth.random_constellation(4, seed_offset=5, cn0_dbhz=50.0)
    x = synth.gps_l1_iq(fs, nblk * N * d, sats, seed_offset=5)
    prns = np.array([s.prn for s in sats])
    codes = np.stack([synth.gps_ca_sampled(p, fs // d) for p in prns])
    acq = gsdr.Acquisition(fs // d, N, 10000, 250, pfa=0.01, max_prns=len(prns), max_blocks=nblk)
    acq.set_local_codes(codes, prns)
    src = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, 1 << 15, 1 << 14)
    dec = gsdr.Decimator(src, d, designed_taps(d), 4 * N, 3 * N)
    try:
        src.push(x, 0)
        head = dec.advance()
        assert head == nblk * N
        r_ring = acq.run_stream(dec.output, 0, nblk, stamp0=N)
        y = dec.output.read(0, nblk * N)
        r_host = acq.run(y, nblk, stamp0=N)
        assert r_ring.tobytes() == r_host.tobytes()
        assert np.all(r_ring["positive"].max(axis=0) == 1)  # 50 dB-Hz: each PRN found in the decimated stream
    finally:
        dec.close()
        src.close()
        acq.close()


def test_golden_capture_decimated(gps_capture):
    """E. The reference's 4 Msps capture decimated by 2 with the 9 designed taps: both
    1 ms blocks give code phase 265 and Doppler 1700 Hz at 2 Msps (the oracle's
    pcps.acquire on the fp64-decimated capture gives the same).  Mapped back to the input
    rate, 265 * 2 - 4 = 526 is within one decimated sample of the 524 that
    gps_l1_ca_pcps_acquisition_test.cc expects, and |1700 - 1680| <= 666."""
    assert len(gps_capture) == 8000
    d, taps = 2, designed_taps(2)
    assert len(taps) == 9
    acq = gsdr.Acquisition(2000000, 2000, 5000, 100, pfa=0.0, max_prns=1, max_blocks=2)
    acq.set_local_codes(synth.gps_ca_sampled(1, 2000000)[None, :], np.array([1]))
    src = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, 1 << 14, 1 << 13)
    dec = gsdr.Decimator(src, d, taps, 4096, 4096)
    try:
        src.push(gps_capture, 0)
        assert dec.advance() == 4000
        res = acq.run_stream(dec.output, 0, 2, stamp0=2000)
        for b in range(2):
            r = res[b, 0]
            assert int(r["code_phase"]) == 265 and int(r["doppler_hz"]) == 1700, (b, r)
            latency = (len(taps) - 1) // 2
            assert abs(int(r["code_phase"]) * d - latency - 524) <= d
            assert abs(int(r["doppler_hz"]) - 1680) <= 666
    finally:
        dec.close()
        src.close()
        acq.close()


def test_errors():
    """F."""
    L = gsdr.load()
    taps = designed_taps(2)
    src = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, 4096, 2048)
    dec = gsdr.Decimator(src, 2, taps, 1024, 512)
    try:
        # the output ring is the decimator's: no host push
        with pytest.raises(gsdr.GsdrError) as e:
            dec.output.push(np.zeros(8, np.complex64), 0)
        assert e.value.code == gsdr.GSDR_E_STATE
        for dd, tt, code in ((0, taps, gsdr.GSDR_E_ARG), (2, np.zeros(0, np.float32), gsdr.GSDR_E_ARG),
                             (65, taps, gsdr.GSDR_E_UNSUPPORTED), (2, np.zeros(1025, np.float32), gsdr.GSDR_E_UNSUPPORTED)):
            with pytest.raises(gsdr.GsdrError) as e:
                gsdr.Decimator(src, dd, tt, 1024, 512)
            assert e.value.code == code, (dd, len(tt))
        # null arguments
        h = ctypes.c_void_p()
        tp = ctypes.c_void_p(taps.ctypes.data)
        assert L.gsdr_decim_create(None, 2, tp, len(taps), 1024, 512, ctypes.byref(h)) == gsdr.GSDR_E_ARG
        assert L.gsdr_decim_create(src._h, 2, None, len(taps), 1024, 512, ctypes.byref(h)) == gsdr.GSDR_E_ARG
        assert L.gsdr_decim_create(src._h, 2, tp, len(taps), 1024, 512, None) == gsdr.GSDR_E_ARG
        assert L.gsdr_decim_advance(None, None) == gsdr.GSDR_E_ARG
        assert L.gsdr_decim_output(dec._h, None) == gsdr.GSDR_E_ARG
        assert L.gsdr_stream_read(None, 0, 1, None) == gsdr.GSDR_E_ARG
        # (the output ring is created on the source's device, so a decimator cannot span
        # two devices; a consumer on another device is refused by the consumer, as for any ring)
        # nothing pushed: nothing to do
        assert dec.advance() == 0
        # pushed more than the source's capacity past the cursor: an error, no fault
        x = np.zeros(4096, np.complex64)
        src.push(x, 0)
        assert dec.advance() == 2048
        src.push(x, 4096)
        src.push(x[:16], 8192)
        with pytest.raises(gsdr.GsdrError) as e:
            dec.advance()
        assert e.value.code == gsdr.GSDR_E_STATE
        assert "source ring" in str(e.value)
        # reads outside the ring are refused
        with pytest.raises(gsdr.GsdrError):
            dec.output.read(0, 1)
        assert len(dec.output.read(2048 - 16, 16)) == 16
    finally:
        dec.close()
        src.close()
