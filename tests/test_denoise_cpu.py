"""The delay-domain pilot denoiser on the CPU: properties of its NumPy restatement (tests/denoise_ref.py), the end-to-end gain
through the oracle, and the façade's refusals, which are raised before any GPU work.

Channels are `h[n] - h[n-2]` of Gaussian taps of amplitude exp(-n / decay), unit energy: no response at DC and Nyquist,
where no pilot is sent.  SNR is the pilot symbols' power over the noise variance."""
import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import denoise_ref as DR

N, K = 1024, 511


def known(seed=5):
    rng = np.random.default_rng(seed)
    return orc.qpsk_table()[0][rng.integers(0, 4, size=K)]


def pilots(rng, h, kn, P, snr_db):
    """P received copies of the pilot symbol (no prefix: the convolution is circular) and the true response on bins 1 .. K."""
    X = np.zeros(N // 2 + 1, dtype=complex)
    X[1:N // 2] = kn
    H = np.fft.rfft(h, N)
    clean = np.fft.irfft(X * H, N)
    sigma = np.sqrt(np.mean(clean ** 2) / 10.0 ** (snr_db / 10.0)) if np.isfinite(snr_db) else 0.0
    return clean[None, :] + sigma * rng.standard_normal((P, N)), H[1:N // 2]


def gain_db(ntaps, decay, seed, P=2, snr_db=10.0):
    rng = np.random.default_rng(seed)
    kn = known()
    xp, H = pilots(rng, DR.sparse_channel(rng, ntaps, decay), kn, P, snr_db)
    out, rep, _ = DR.denoise_row(xp, kn)
    ls = np.fft.rfft(DR.pilot_sum(xp))[1:N // 2] / (P * kn)
    dn = np.fft.rfft(out)[1:N // 2] / (P * kn)
    return 10.0 * np.log10(np.mean(np.abs(ls - H) ** 2) / np.mean(np.abs(dn - H) ** 2)), rep


@pytest.mark.parametrize("ntaps,decay,need", [(24, 5.0, 6.0), (256, 51.2, 2.0)])
def test_mse_gain_on_every_seed(ntaps, decay, need):
    got = [gain_db(ntaps, decay, seed) for seed in range(40)]
    gains = np.array([g for g, _ in got])
    print(f"{ntaps} taps, decay {decay}: gain over LS min {gains.min():.1f} dB, mean {gains.mean():.1f} dB; "
          f"kept {min(r[1] for _, r in got):.0f} .. {max(r[1] for _, r in got):.0f}")
    assert all(r[4] == 1 for _, r in got)
    assert gains.min() >= need


def test_noiseless_forced_and_nan_rows_pass_through():
    rng = np.random.default_rng(3)
    kn = known()
    h = DR.sparse_channel(rng, 24, 5.0)
    clean, _ = pilots(rng, h, kn, 2, np.inf)
    out, rep, _ = DR.denoise_row(clean, kn)
    assert rep[0] == 0.0 and rep[1] > N // 4 and rep[4] == 0
    assert np.array_equal(out.view(np.uint8), DR.pilot_sum(clean).view(np.uint8))
    noisy, _ = pilots(rng, h, kn, 2, 10.0)
    applied, rep_a, _ = DR.denoise_row(noisy, kn)
    assert rep_a[4] == 1 and not np.array_equal(applied, DR.pilot_sum(noisy))
    out, rep, _ = DR.denoise_row(noisy, kn, max_kept=int(rep_a[1]) - 1)          # forced: one tap more than allowed
    assert rep[4] == 0 and np.array_equal(rep[:4], rep_a[:4])
    assert np.array_equal(out.view(np.uint8), DR.pilot_sum(noisy).view(np.uint8))
    bad = noisy.copy()
    bad[1, 77] = np.nan
    out, rep, _ = DR.denoise_row(bad, kn)
    assert np.isnan(rep[0]) and rep[1:].tolist() == [0, -1, 0, 0]
    assert np.array_equal(out.view(np.uint8), DR.pilot_sum(bad).view(np.uint8))


def test_ragged_packet_is_a_zero_row():
    p = DR.small_params(np.random.default_rng(1).integers(0, 2, size=2 * K))
    r, starts, _ = DR.noisy_stream(p, seed=2, F=2, tail=0)
    r = r[: starts[1] + p.M * p.S - 1]                             # the second packet runs one sample past the stream
    out, rep, plain, _ = DR.denoise_frames(r, starts, p.N, p.CP, p.P, p.D, p.known_symbols())
    assert rep[0, :, 4].tolist() == [1, 1]
    assert not out[1].any() and not plain[1].any() and rep[1].tolist() == [[0, 0, -1, 0, 0]] * 2


@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_kernel_cases_keep_clear_of_the_threshold(N):
    """The condition under which tests/test_denoise_gpu.py compares keep decisions as integers, by the restatement alone:
    no tap of any kernel case (P in 2, 3, 9; four sample storages) lies within 1e-6 (relative) of the keep threshold."""
    for P in (2, 3, 9):
        for dtype in ("float64", "float32", "int16", "uint8"):
            p, x, starts = DR.kernel_case(N, P, dtype, seed=N + P)
            margin = DR.denoise_frames(x, starts, p.N, p.CP, p.P, p.D, p.known_symbols())[3]
            print(f"N {N} {dtype} P {P}: nearest tap to the threshold {margin:.1e}")
            assert margin >= 1e-6, (P, dtype)


def test_delay_spread_of_a_planted_channel():
    """One causal tap at 17 and one precursor at N - 3, of opposite signs (both odd: no response at DC and Nyquist); 5 sigma,
    so that no noise tap survives (1024 taps x 5.7e-7)."""
    rng = np.random.default_rng(11)
    kn = known()
    h = np.zeros(N)
    h[17], h[N - 3] = 1.0, -1.0
    xp, _ = pilots(rng, h, kn, 2, 10.0)
    _, rep, _ = DR.denoise_row(xp, kn, tau=25.0)
    assert rep[1:].tolist() == [2, 17, 3, 1]


def errors(p, seed, ntaps):
    r, starts, bits = DR.noisy_stream(p, seed, ntaps=ntaps)
    plain = int(np.sum(orc.demod_frames(r, starts, p)["bits"] != bits))
    r2, rep = DR.emulate(r, starts, p)
    assert rep[:, :, 4].all()
    return plain, int(np.sum(orc.demod_frames(r2, starts, p)["bits"] != bits))


def test_end_to_end_through_the_oracle():
    """N = 1024, CP = 64, P = 2, D = 12, F = 4, carriers 20 .. 399, 24-tap channel, 6 dB SNR on the body, 4 seeds: the bit errors
    with denoised pilots, summed over the seeds, are below 0.8 x those with plain pilots."""
    p = DR.small_params(np.random.default_rng(1).integers(0, 2, size=2 * K))
    got = [errors(p, seed, 24) for seed in range(4)]
    plain, den = sum(a for a, _ in got), sum(b for _, b in got)
    print(f"bit errors plain / denoised per seed {got}: ratio {den / plain:.3f} of {4 * 4 * p.D * p.C * p.mu} bits per leg")
    assert den < 0.8 * plain


# ---- the façade's refusals: before any GPU work ----------------------------------------------------------------------
def rx_of(**kw):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding=kw.pop("encoding", "None"), no_pilots=kw.pop("no_pilots", 2), packet_length=4)
    rx.channel_denoising = True
    for k, v in kw.items():
        setattr(rx, k, v)
    return rx


def test_facade_defaults():
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2")
    assert rx.channel_denoising is False and rx.denoise_threshold == 9.0 and rx.last_denoise_report is None
    assert rx._chain().denoise is None and rx._chain().check_denoise() is None


@pytest.mark.parametrize("call", ["receive", "receive_diversity"])
def test_facade_refusals(call):
    r = np.zeros(5000)
    arg = (lambda: [r, r]) if call == "receive_diversity" else (lambda: r)
    with pytest.raises(ValueError, match="channel_denoising.*fused_llr"):
        getattr(rx_of(encoding="QCLDPC-1/2", fused_llr=True), call)(arg())
    with pytest.raises(ValueError, match="no_pilots >= 2"):
        getattr(rx_of(no_pilots=1), call)(arg())
    for bad in (0.0, -9.0, float("nan"), float("inf"), "9", None, True):
        with pytest.raises(ValueError, match="denoising threshold"):
            getattr(rx_of(denoise_threshold=bad), call)(arg())
    with pytest.raises(NotImplementedError, match="piece-wise host path"):
        getattr(rx_of(host_chunk_samples=1 << 22), call)(arg())
