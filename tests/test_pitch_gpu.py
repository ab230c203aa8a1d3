"""GPU: mvn_pitch_frames through ``ops.pitch`` against the float64 reference of tests/pitch_reference.py on
3 rows of 2000 samples at three settings -- tau_max below one wave, off a multiple of 64, and beyond 256 lanes; a win that
is no multiple of 64; more frames than one workgroup; edge frames that reach into the zero padding -- the planted known
answers, and the bit-exact invariants.

Tolerances.  c: |c - c_ref| <= rtol c_ref + atol with rtol = 4 (win + tau_max) 2^-24 (``R.cmnd_rtol``) and atol =
``R.CMND_ATOL``, 4 x the largest deviation measured on these inputs; 0 where c carries no error
(``R.cmnd_tolerance``).  The pick is compared on the frames whose decision every c within that tolerance shares
(``R.safe_frames``; at most 5 % of a row's frames may be left out), and there ``period`` within ``R.period_bound``: the
tolerance carried through the parabola's quotient plus its fp32 rounding."""
import functools

import numpy as np
import pytest
import torch

import pitch_reference as R
from helpers import DEV
from movenet_amd import ops

pytestmark = pytest.mark.gpu


def _kw(setting, **more):
    win, hop, tau_min, tau_max = setting
    return dict(win=win, hop=hop, tau_min=tau_min, tau_max=tau_max, threshold=R.THRESHOLD, **more)


@functools.lru_cache(maxsize=None)
def _case(setting):
    """(rows float32, reference, tolerance, safe, period bound, the kernel's output) of one setting, made once."""
    win, hop, tau_min, tau_max = setting
    x = R.make_rows(tau_min, tau_max)
    ref = R.track(x, win, hop, tau_min, tau_max, R.THRESHOLD)
    tol = R.cmnd_tolerance(x, ref["cmnd"], win, hop, tau_max)
    safe, bound = R.safe_frames(ref, tol, tau_min, tau_max, R.THRESHOLD)
    got = {k: v.cpu().numpy() for k, v in ops.pitch(torch.from_numpy(x).to(DEV), **_kw(setting, cmnd=True)).items()}
    return x, ref, tol, safe, bound, got


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_cmnd_against_float64(setting):
    x, ref, tol, _, _, got = _case(setting)
    F = R.frames_of(R.SAMPLES, setting[1])
    assert got["cmnd"].shape == (R.ROWS, F, setting[3] + 1) and got["cmnd"].dtype == np.float32
    dev = np.abs(got["cmnd"].astype(np.float64) - ref["cmnd"])
    excess = dev - R.cmnd_rtol(setting[0], setting[3]) * np.abs(ref["cmnd"])
    print(f"setting {setting}: largest |c - c_ref| = {dev.max():.3e}, largest relative = "
          f"{(dev / np.abs(ref['cmnd'])).max():.3e} (rtol {R.cmnd_rtol(setting[0], setting[3]):.3e}), largest excess over "
          f"rtol c = {excess.max():.3e}")
    assert np.all(np.isfinite(got["cmnd"])) and np.all(got["cmnd"][:, :, 0] == 1.0)
    assert np.all(dev <= tol), f"largest deviation over its tolerance: {(dev - tol).max():.3e}"


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_pick_and_period_on_the_safe_frames(setting):
    x, ref, tol, safe, bound, got = _case(setting)
    unsafe = (~safe).sum(axis=1)
    print(f"setting {setting}: unsafe frames per row {unsafe.tolist()} of {safe.shape[1]}; voiced per row "
          f"{ref['voiced'].sum(axis=1).tolist()}")
    assert np.all(unsafe <= 0.05 * safe.shape[1])
    voiced = got["period"] > 0
    assert np.array_equal(voiced[safe], ref["voiced"][safe])
    assert np.all(got["period"][~voiced] == 0.0)
    # tau*: aper is c(tau*), so on a safe frame it is the kernel's own c at the reference's tau*, bit for bit; and the
    # refined period lies within 1/2 of it
    at_ref = np.take_along_axis(got["cmnd"], ref["tau"][:, :, None], axis=2)[:, :, 0]
    assert np.array_equal(got["aper"][safe], at_ref[safe])
    both = safe & ref["voiced"]
    assert np.all(np.abs(got["period"][both] - ref["tau"][both]) <= 0.5)
    err = np.abs(got["period"].astype(np.float64) - ref["period"])
    print(f"  largest |period - period_ref| on safe voiced frames = {err[both].max() if both.any() else 0.0:.3e}, "
          f"largest bound = {bound[both].max() if both.any() else 0.0:.3e}")
    assert np.all(err[both] <= bound[both])


def test_planted_known_answers():
    n = 1200
    sine = np.sin(2 * np.pi * np.arange(n) / 37.3).astype(np.float32)
    const = np.full(n, 0.25, np.float32)
    noise = (np.random.default_rng(3).standard_normal(n) * 0.3).astype(np.float32)
    x = torch.from_numpy(np.stack([sine, const, noise])).to(DEV)
    # frames whose L = 256 + 100 samples lie inside the row: 64 j - 178 >= 0 and 64 j + 178 <= 1200
    inside = slice(3, 16)
    for tau_max in (60, 100):  # 100 >= 2 x 37.3: the pick is the first dip, not the octave below
        got = {k: v.cpu().numpy() for k, v in ops.pitch(x, win=256, hop=64, tau_min=8, tau_max=tau_max,
                                                        cmnd=True).items()}
        assert np.all(np.abs(got["period"][0, inside] - 37.3) <= 1.5)
        assert np.all(got["cmnd"][1, inside] == 1.0) and np.all(got["period"][1, inside] == 0.0)
        assert np.all(got["aper"][1, inside] == 1.0)
        assert np.all(got["period"][2] == 0.0) and np.all(got["aper"][2] > 0.15)
        assert np.all(np.isfinite(got["cmnd"]))


@pytest.mark.parametrize("Q", [64, 256])
def test_indices_track_as_their_decoded_waveform_bit_for_bit(Q):
    setting = R.SETTINGS[1]
    g = torch.Generator().manual_seed(Q)
    t = torch.arange(R.SAMPLES, dtype=torch.float64)
    wave = 0.5 * torch.sin(2 * torch.pi * t / 47.3)[None] + 0.05 * torch.randn(2, R.SAMPLES, generator=g, dtype=torch.float64)
    idx = ops.mu_law_encode(wave.float().clamp(-1, 1).to(DEV), Q)
    idx[0, 5], idx[1, 777], idx[1, 778] = -3, Q, 10 ** 6  # out of range: a 0.0 sample
    decoded = ops.mu_law_decode(idx, Q)
    decoded[0, 5] = decoded[1, 777] = decoded[1, 778] = 0.0
    a, b = ops.pitch(idx, Q, **_kw(setting, cmnd=True)), ops.pitch(decoded, **_kw(setting, cmnd=True))
    for k in ("period", "aper", "cmnd"):
        assert torch.equal(a[k], b[k]), k
    assert bool((a["period"] > 0).any())
    assert torch.equal(ops.pitch(idx.long(), Q, **_kw(setting))["period"], a["period"])


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_rows_alone_repeats_and_no_cmnd_give_the_same_bits(setting):
    x = torch.from_numpy(_case(setting)[0]).to(DEV)
    full = ops.pitch(x, **_kw(setting, cmnd=True))
    again = ops.pitch(x, **_kw(setting, cmnd=True))
    lean = ops.pitch(x, **_kw(setting))
    assert "cmnd" not in lean
    for k in ("period", "aper"):
        assert torch.equal(full[k], again[k]) and torch.equal(full[k], lean[k]), k
    assert torch.equal(full["cmnd"], again["cmnd"])
    for b in range(R.ROWS):
        alone = ops.pitch(x[b:b + 1], **_kw(setting, cmnd=True))
        for k in ("period", "aper", "cmnd"):
            assert torch.equal(alone[k][0], full[k][b]), (k, b)


def test_a_non_finite_sample_stays_inside_the_frames_that_cover_it():
    setting = R.SETTINGS[0]
    win, hop, _, tau_max = setting
    x = torch.from_numpy(_case(setting)[0]).to(DEV).clone()
    clean = ops.pitch(x, **_kw(setting))
    x[0, 1000] = float("nan")
    x[1, 400] = float("inf")
    dirty = ops.pitch(x, **_kw(setting))
    L = win + tau_max
    for b, at in ((0, 1000), (1, 400)):
        covers = torch.tensor([j * hop - L // 2 <= at < j * hop - L // 2 + L
                               for j in range(R.frames_of(R.SAMPLES, hop))], device=DEV)
        assert bool(covers.any()) and not bool(covers.all())
        for k in ("period", "aper"):
            assert torch.equal(dirty[k][b][~covers], clean[k][b][~covers]), (k, b)
    assert torch.equal(dirty["period"][2], clean["period"][2])


def test_nothing_outside_the_outputs_is_written():
    """The C ABI on outputs that sit inside larger poisoned buffers."""
    from movenet_amd import _native as N
    setting = R.SETTINGS[2]
    win, hop, tau_min, tau_max = setting
    x = torch.from_numpy(_case(setting)[0]).to(DEV)
    B, T = x.shape
    F = R.frames_of(T, hop)
    pad, poison = 4096, -1234.5
    sizes = {"period": B * F, "aper": B * F, "cmnd": B * F * (tau_max + 1)}
    bufs = {k: torch.full((n + 2 * pad,), poison, dtype=torch.float32, device=DEV) for k, n in sizes.items()}
    lib = N.lib()
    n = int(lib.mvn_pitch_scratch_floats(B, T, win, tau_max))
    scratch = torch.empty(n, dtype=torch.float32, device=DEV)
    ptr = {k: v.data_ptr() + 4 * pad for k, v in bufs.items()}
    N.check(lib.mvn_pitch_frames(None, x.data_ptr(), B, T, 0, win, hop, tau_min, tau_max, R.THRESHOLD, ptr["period"],
                                 ptr["aper"], ptr["cmnd"], scratch.data_ptr(), n,
                                 torch.cuda.current_stream(torch.device(DEV)).cuda_stream), "mvn_pitch_frames")
    torch.cuda.synchronize()
    want = ops.pitch(x, **_kw(setting, cmnd=True))
    for k, size in sizes.items():
        assert bool((bufs[k][:pad] == poison).all()) and bool((bufs[k][pad + size:] == poison).all()), k
        assert torch.equal(bufs[k][pad:pad + size], want[k].reshape(-1)), k


def test_ops_refusals_on_the_gpu():
    x = torch.zeros(2, 100, device=DEV)
    kw = dict(win=64, hop=16, tau_min=4, tau_max=40)
    for bad in (x[0], x.double(), x.bool()):
        with pytest.raises(ValueError, match="indices_or_wave"):
            ops.pitch(bad, **kw)
    with pytest.raises(ValueError, match="classes"):
        ops.pitch(x.int(), **kw)
    with pytest.raises(ValueError, match="classes"):
        ops.pitch(x.int(), 1, **kw)
    with pytest.raises(ValueError, match="tau_min"):
        ops.pitch(x, **{**kw, "tau_min": 41})
    out = ops.pitch(x, **kw)
    assert out["period"].shape == (2, 7) and not out["period"].any() and bool((out["aper"] == 1.0).all())
