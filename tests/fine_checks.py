"""Float64 restatement of pcps_acquisition_fine_doppler_cc::estimate_Doppler
(pcps_acquisition_fine_doppler_cc.cc:346-419) and the inputs the fine-Doppler tests share.

Written from the reference's text:
  :363-371  the replica, aligned by std::rotate(c, c + (N - shift), c + N - 1) -- the range
            ends at N - 1, so the last sample stays and shift 0 and 1 change nothing;
  :373-376  ten copies of that row;
  :378-381  code wipe-off, zero padding to 80 N points, one forward FFT;
  :385-388  |X|^2 and its first maximum (volk_gnsssdr_32f_index_max_32u);
  :394-404  fftFreqBins: float operands, the literals 2.0 make the product and the quotient
            doubles, the store into the float vector rounds once;
  :407-416  accepted when std::abs(freq - Acq_doppler_hz) < 1000 (in double).
"""
import functools

import numpy as np

from gsdr import synth

PRN_REPLICAS = 10
ZERO_PADDING = 8
MIN_MARGIN = 1e-3   # every comparison first pins the best bin this far above the second best
RTOL = 1e-4         # the project's acquisition tolerance, relative to the maximum


def rotate_replica(code, shift):
    """std::rotate(c, c + (N - shift), c + N - 1) when shift != 0 (:365-371)."""
    c = np.array(code)
    n = len(c)
    if shift != 0:
        head = c[:n - 1].copy()
        mid = n - shift
        c[:n - 1] = np.concatenate([head[mid:], head[:mid]])
    return c


def wiped(x, code, shift):
    """fft_operator's input before the padding: d_10_ms_buffer .* ten aligned replicas."""
    n = len(code)
    assert len(x) == PRN_REPLICAS * n
    rep = np.tile(rotate_replica(np.asarray(code, np.complex128), shift), PRN_REPLICAS)
    return np.asarray(x, np.complex128) * rep


def padded_spectrum(y):
    buf = np.zeros(ZERO_PADDING * len(y), np.complex128)
    buf[:len(y)] = y
    return np.fft.fft(buf)


def residue_spectrum(y):
    """The same 8 L bins as eight L-point transforms of y times a phase ramp:
    X[8 q + r] = FFT_L(y[n] e^{-2 pi i n r / M})[q]."""
    L = len(y)
    M = ZERO_PADDING * L
    n = np.arange(L, dtype=np.int64)
    X = np.zeros(M, np.complex128)
    for r in range(ZERO_PADDING):
        X[r::ZERO_PADDING] = np.fft.fft(y * np.exp(-2j * np.pi * ((n * r) % M) / M))
    return X


def freq_bin(k, fs, M):
    """fftFreqBins[k] (:394-404)."""
    fsf = np.float64(np.float32(fs))
    half_m = np.float64(np.float32(M)) / 2.0
    if k < M // 2:
        return np.float32(((fsf / 2.0) * np.float64(np.float32(k))) / half_m)
    return np.float32(((-fsf / 2.0) * np.float64(np.float32(M - k))) / half_m)


def estimate_doppler(x, code, shift, coarse_hz, fs):
    """-> dict(spectrum (float64 |X|^2), index, peak, freq_hz (float32), accepted, doppler_hz,
    margin = (best - second best) / best)."""
    p = np.abs(padded_spectrum(wiped(x, code, shift))) ** 2
    M = len(p)
    k = int(np.argmax(p))  # the first maximum
    two = np.partition(p, M - 2)[M - 2:]
    freq = freq_bin(k, fs, M)
    coarse = float(np.float32(coarse_hz))
    ok = abs(float(freq) - coarse) < 1000
    return {"spectrum": p, "index": k, "peak": float(p[k]), "freq_hz": freq, "accepted": int(ok),
            "doppler_hz": float(freq) if ok else coarse, "margin": float((two[1] - two[0]) / two[1])}


# ---- shared inputs: 10 N samples from t0 = 2 N (inside one navigation bit), three satellites
# at 45-47 dB-Hz whose Dopplers are whole fine bins (12.5 Hz at each of these rates), and one
# absent PRN.  Per satellite: (prn, fine bin k, code phase in samples).  Over the cases the
# peaks cover the code phases 0, 1, 2, N - 1 and mid-row values, both signs of the frequency
# and every residue of the peak's bin index mod 8:
#   k mod 8 = 0 (80), 7 (-161), 1 (241) | 2 (162), 5 (-83), 3 (323) | 4 (100), 6 (-242), 0 (-400)
CASES = {
    "lds20000": dict(fs=2000000, N=2000, plan=(20000, 0, 20000), absent=(29, 1500, -1750.0),
                     sats=[(3, 80, 0), (11, -161, 1), (22, 241, 777)]),
    "four20480": dict(fs=2048000, N=2048, plan=(20480, 10, 2048), absent=(30, 5, 500.0),
                      sats=[(5, 162, 2047), (14, -83, 1), (27, 323, 1000)]),
    "four40000": dict(fs=4000000, N=4000, plan=(40000, 10, 4000), absent=(31, 2000, 2500.0),
                      sats=[(7, 100, 2741), (17, -242, 2), (25, -400, 3999)]),
    # the 1024-lane four-step: 10 x 16000, and 25 x 10000 at 25 Msps, whose peaks lie at bins
    # where an all-float evaluation of fftFreqBins differs from the reference's (43: 537.5 Hz
    # against 537.50006), so the bit-equal frequency shows which one the engine computes
    "four160000": dict(fs=16000000, N=16000, plan=(160000, 10, 16000), absent=(28, 9000, 0.0),
                       sats=[(2, 120, 5), (13, -203, 8000), (21, 333, 15999)]),
    "four250000": dict(fs=25000000, N=25000, plan=(250000, 25, 10000), absent=(32, 12345, 250.0),
                       sats=[(6, 43, 24999), (15, -45, 3), (23, 161, 11111)]),
}
CN0 = (45.0, 46.0, 47.0)


class FineCase:
    def __init__(self, name):
        c = CASES[name]
        self.name, self.fs, self.N, self.plan = name, c["fs"], c["N"], c["plan"]
        self.L, self.M = PRN_REPLICAS * self.N, ZERO_PADDING * PRN_REPLICAS * self.N
        self.step = self.fs / self.M
        assert self.step == 12.5
        sats = []
        for i, (prn, k, shift) in enumerate(c["sats"]):
            # the sampled replica's sample i is the chip at time (i + 1) / fs (synth.gps_ca_sampled),
            # so a code that starts shift - 1 samples into each block of N correlates best at shift
            sats.append(synth.Satellite(prn, k * self.step, ((shift - 1) % self.N) * 1023.0 / self.N, CN0[i],
                                        phase=0.4 + 1.1 * i))
        self.x = synth.gps_l1_iq(self.fs, self.L, sats, seed_offset=len(name), t0_samples=2 * self.N)
        self.prns = [s[0] for s in c["sats"]] + [c["absent"][0]]
        self.codes = np.stack([synth.gps_ca_sampled(p, self.fs) for p in self.prns])
        assert self.codes.shape == (4, self.N)
        # requests (code_phase, coarse_doppler_hz, code_slot): the three satellites with the
        # coarse Doppler of a 250 Hz grid, then the absent PRN
        self.requests = [(shift, float(np.round(k * self.step / 250.0) * 250.0), slot)
                         for slot, (_, k, shift) in enumerate(c["sats"])]
        self.requests.append((c["absent"][1], c["absent"][2], 3))
        self.true_index = [k % self.M for _, k, _ in c["sats"]]

    def items(self, item_type):
        """The window as the handle's items, and as the complex samples the engine reads."""
        if item_type == 0:
            return self.x, self.x
        if item_type == 1:
            raw = synth.to_cshort(self.x, 1000.0)
        else:
            raw = synth.to_ibyte(self.x, 20.0)
        return raw, raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)

    @functools.lru_cache(maxsize=None)
    def reference(self, i, item_type=0, coarse=None):
        """estimate_doppler of request i (the coarse Doppler replaced when given)."""
        shift, c0, slot = self.requests[i]
        return estimate_doppler(self.items(item_type)[1], self.codes[slot], shift, c0 if coarse is None else coarse,
                                self.fs)


@functools.lru_cache(maxsize=None)
def fine_case(name):
    return FineCase(name)
