"""Exact integer probe of the stand-alone multicorrelator (not a test module).

With rem_carr = carr_step = carr_rate = 0 the rotator is exactly (1, 0) on the host
model, the device model and in the oracle: the angles are +-0, sincosf(0) is exact
and the phasor recursion multiplies by (1, 0).  With integer IQ in [-7, 7] and an
integer replica in [-15, 15] every product and every partial sum, in any order, is
an integer below 2^24, so fp32 accumulation is exact and the GPU's taps must equal
the int64 sums below bit for bit.  A wrong code index, a wrong LDS span, a lost
chunk partial or a stale output then changes the value instead of hiding below a
tolerance on +-1 chips.

The indices come from the oracle's restatement of the reference resamplers
(volk.resampler_index; volk.high_dyn_resampler_32f_xn on code = arange(L)).
Complex replicas with the high-dynamics resampler have no reference implementation
(Cpu_Multicorrelator has no high-dynamics path), so the probe refuses them.

Read by test_gpu_corr_paths.py (GPU against these sums) and test_oracle_corr.py
(the helpers alone, no GPU).
"""
import numpy as np
import torch  # before libgsdr.so is loaded, as in test_gpu_corr.py: both bring a HIP runtime

import gsdr
from gsdr import synth
from oracle import volk

CHUNK = 4096     # samples per workgroup (kChunk, corr.hip)
SPAN_CAP = 4096  # replica entries a chunk stages in LDS (kSpanCap)
EXACT_LIMIT = 1 << 24
GENERIC, AVX = gsdr.ASSOC_GENERIC, gsdr.ASSOC_AVX

# Non-dyadic shifts, remainder and step for which the two float associations of the
# code index, floor((step*n + shift) - rem) and floor(step*n + (shift - rem)),
# disagree at 1 index of N = 4000 and at 4 of N = 8197, found by a seeded search
# over rem in [-0.5, 0.5) and step = 1023/4000 (1 +- 1e-4) that kept the first draw
# whose probe sums differ at both lengths; expected_both_assocs asserts it on every
# use.  For the dyadic shifts of test_gpu_corr.py (+-0.5, +-0.25, 0) they never
# disagree.
AG_SHIFTS = np.array([-0.6, -0.15, 0.1, 0.15, 0.6], np.float32)
AG_REM = float(np.float32(-0.23530487716197968))
AG_STEP = float(np.float32(0.25575050711631775))
AG_L = 1023


def f32(v):
    return float(np.float32(v))


def probe_iq(n, seed):
    """(n, 2) int64, I and Q uniform integers in [-7, 7]."""
    return np.random.default_rng(1000 + seed).integers(-7, 8, size=(n, 2)).astype(np.int64)


def probe_code(L, seed, cplx=False):
    """Integer replica in [-15, 15]: float32, or complex64 with both parts drawn."""
    c = np.random.default_rng(2000 + seed).integers(-15, 16, size=(L, 2))
    if cplx:
        return (c[:, 0] + 1j * c[:, 1]).astype(np.complex64)
    return c[:, 0].astype(np.float32)


def iq_items(iq, item_type=gsdr.ITEM_GR_COMPLEX):
    """The integer IQ as host items of item_type (cshort and ibyte hold it natively)."""
    if item_type == gsdr.ITEM_GR_COMPLEX:
        return (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64)
    dt = np.int16 if item_type == gsdr.ITEM_CSHORT else np.int8
    return np.ascontiguousarray(iq.astype(dt).reshape(-1))


class Chan:
    """One channel's configuration: replica, tap shifts, high-dynamics resampler."""

    def __init__(self, code, shifts, high_dyn=False):
        self.code = np.asarray(code)
        self.shifts = np.ascontiguousarray(shifts, np.float32)
        self.high_dyn = bool(high_dyn)
        self.cplx = np.iscomplexobj(self.code)
        # out of scope: the reference has no complex-code high-dynamics correlator
        assert not (self.cplx and self.high_dyn), "complex codes + high dynamics has no reference"

    @property
    def K(self):
        return len(self.shifts)

    @property
    def L(self):
        return len(self.code)


def indices(ch, rem, step, N, assoc=AVX, rate=0.0):
    """(K, N) int64 code indices of the reference resampler for this channel."""
    if N == 0:
        return np.zeros((ch.K, 0), np.int64)
    if ch.high_dyn:
        ramp = np.arange(ch.L, dtype=np.float32)  # exact: L < 2^24
        return volk.high_dyn_resampler_32f_xn(ramp, rem, step, rate, ch.shifts, N).astype(np.int64)
    return volk.resampler_index(rem, step, ch.shifts, ch.L, N, assoc=assoc).astype(np.int64)


def raw_indices(ch, rem, step, n, assoc=AVX):
    """Unwrapped floor(...) of the non-high-dynamics index at samples n (float32, no FMA):
    what the kernel derives a chunk's replica span from."""
    n = np.asarray(n)
    a = np.float32(step) * n.astype(np.float32)
    s = ch.shifts[:, None]
    r = np.float32(rem)
    t = (a[None, :] + s) - r if assoc == GENERIC else a[None, :] + (s - r)
    assert t.dtype == np.float32
    return np.floor(t).astype(np.int64)


def chunk_spans(ch, rem, step, N, assoc=AVX):
    """Replica entries spanned by each CHUNK of an N-sample job (step > 0)."""
    spans = []
    for n0 in range(0, N, CHUNK):
        n1 = min(N, n0 + CHUNK)
        spans.append(int(raw_indices(ch, rem, step, [n1 - 1], assoc).max() -
                         raw_indices(ch, rem, step, [n0], assoc).min() + 1))
    return spans


def expected(iq, ch, idx):
    """int64 correlation of the integer IQ rows with the replica at idx (K, N), as
    complex64.  Asserts that no partial sum in any order can reach 2^24."""
    K, N = idx.shape
    iq = np.asarray(iq, np.int64)
    assert iq.shape == (N, 2)
    parts = np.stack([ch.code.real, ch.code.imag]) if ch.cplx else ch.code[None, :]
    assert np.array_equal(parts, np.rint(parts)), "the probe needs an integer replica"
    parts = parts.astype(np.int64)
    amax = int(np.abs(iq).max()) if N else 0
    cmax = int(np.abs(parts).max())
    assert 2 * N * amax * cmax < EXACT_LIMIT, (N, amax, cmax)
    i, q = iq[:, 0][None, :], iq[:, 1][None, :]
    cr = parts[0][idx]
    if ch.cplx:
        ci = parts[1][idx]
        re, im = (i * cr - q * ci).sum(axis=1), (i * ci + q * cr).sum(axis=1)
    else:
        re, im = (i * cr).sum(axis=1), (q * cr).sum(axis=1)
    assert max(int(np.abs(re).max()), int(np.abs(im).max())) < EXACT_LIMIT
    return (re + 1j * im).astype(np.complex64)


def expected_both_assocs(iq, ch, rem, step, N):
    """{assoc: expected sums}; asserts, on the CPU, that the two associations give
    different sums in at least one tap, so a swapped association cannot pass."""
    e = {a: expected(iq[:N], ch, indices(ch, rem, step, N, assoc=a)) for a in (GENERIC, AVX)}
    assert np.any(e[GENERIC] != e[AVX]), "the associations agree here: the case proves nothing"
    return e


def job(channel, n, offset=0, rem=0.0, step=AG_STEP, rate=0.0):
    """One gsdr.CORR_JOB_DTYPE row of the probe: the carrier terms are all zero."""
    return (channel, n, offset, 0.0, 0.0, 0.0, np.float32(rem), np.float32(step), np.float32(rate))


def job_table(rows):
    t = np.zeros(len(rows), gsdr.CORR_JOB_DTYPE)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def window(iq, offset, n):
    """Samples [offset, offset + n) of iq with zeros outside [0, len(iq)), as the kernel reads them."""
    out = np.zeros((n, 2), np.int64)
    lo, hi = max(offset, 0), min(offset + n, len(iq))
    if hi > lo:
        out[lo - offset:hi - offset] = iq[lo:hi]
    return out


def expected_rows(iq, chans, jobs, assoc=AVX):
    """Per job, the expected first K entries of its output row."""
    rows = []
    for j in jobs:
        ch, n = chans[int(j["channel"])], int(j["n_samples"])
        idx = indices(ch, float(j["rem_code_phase_chips"]), float(j["code_phase_step_chips"]), n, assoc=assoc,
                      rate=float(j["code_phase_rate_step_chips"]))
        rows.append(expected(window(iq, int(j["sample_offset"]), n), ch, idx))
    return rows


# --- inputs of the tolerance tests -----------------------------------------------

SHIFTS5 = np.array([-0.5, -0.25, 0.0, 0.25, 0.5], np.float32)


def strong_signal(fs, N, prn, doppler, seed):
    """cn0 = 55 dB-Hz, code delay 0: the prompt tap is aligned."""
    return synth.gps_l1_iq(fs, N, [synth.Satellite(prn, doppler, 0.0, 55.0)], seed_offset=seed)


def complex_code(prn):
    """A complex replica whose imaginary part is the C/A code (gps_ca_sampled is
    (0, +-1)) and whose real part is a delayed half-amplitude copy."""
    code = synth.gps_ca_sampled(prn, 1023000).astype(np.complex64)
    return (code + 0.5 * np.roll(code, 3).imag).astype(np.complex64)


# --- GPU side -------------------------------------------------------------------


def correlator(chans, max_len, max_taps, assoc=AVX):
    corr = gsdr.Correlator(len(chans), max_len, max_taps=max_taps)
    corr.set_resampler_assoc(assoc)
    for c, ch in enumerate(chans):
        corr.set_local_code_and_taps(c, ch.code, ch.shifts)
        if ch.high_dyn:
            corr.set_high_dynamics_resampler(c, True)
    return corr


def to_device(host):
    if host.dtype == np.complex64:
        host = host.view(np.float32)
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def launch(corr, jobs, iq_dev, n_items, how="host", item_type=gsdr.ITEM_GR_COMPLEX, epochs=1):
    """One launch of the whole table (or `epochs` launches of equal slices of it for
    how="epochs") into an output pre-filled with NaN, so a row the kernel does not
    write, or writes late, shows.  Returns (len(jobs), max_taps) complex64."""
    jobs = np.ascontiguousarray(jobs, gsdr.CORR_JOB_DTYPE)
    out = torch.full((len(jobs) * corr.max_taps * 2,), float("nan"), dtype=torch.float32, device="cuda")
    jdev = to_device(jobs.view(np.uint8)) if how != "host" else None
    torch.cuda.synchronize()  # the handle runs on a stream of its own
    if how == "host":
        corr.run_batch(jobs, iq_dev.data_ptr(), n_items, out.data_ptr(), item_type=item_type)
    elif how == "device":
        corr.run_batch_device(jdev.data_ptr(), len(jobs), iq_dev.data_ptr(), n_items, out.data_ptr(),
                              item_type=item_type)
    else:
        assert how == "epochs" and len(jobs) % epochs == 0
        corr.run_epochs(jdev.data_ptr(), len(jobs) // epochs, epochs, iq_dev.data_ptr(), n_items, out.data_ptr(),
                        item_type=item_type)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.complex64).reshape(len(jobs), corr.max_taps)


def assert_rows_exact(got, want_rows):
    for j, want in enumerate(want_rows):
        np.testing.assert_array_equal(got[j, :len(want)], want, err_msg="job %d" % j)
