"""GPU: mvn_context_window and mvn_project_features against the three-kernel path they stand for, bit for
bit -- mvn_upsample_features_win over all T columns, mvn_transpose_context, mvn_context_add_global.  Every comparison is
``torch.equal`` on the int32 views (a -0.0 is not a +0.0 here), and every window is written inside a larger allocation
whose bands of sentinel values must come back untouched."""
import functools

import pytest
import torch

from helpers import DEV
from movenet_amd import _native as N
from movenet_amd import ops

pytestmark = pytest.mark.gpu
B, M, T = 3, 5, 1100
SENTINEL = -1234.5
BAND = 4096


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _reference(C, hop, taps):
    """Today's path, once per shape: proj (the up-sampler's scratch), tm (B, T, C) without a label, tm_g with one,
    tm_2g (2 B rows: zeros in the first B rows' vectors) and the inputs."""
    lib = N.lib()
    g = torch.Generator().manual_seed(1000 * C + 10 * hop + taps)
    F = (T - 1) // hop + 1
    mel = torch.randn(B, M, F, generator=g).to(DEV)
    w = (torch.randn(C, M, taps, generator=g) * 0.5).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    glob = torch.randn(B, C, generator=g).to(DEV)
    glob[0, 0] = 0.0
    ld = (T + 3) // 4 * 4
    with torch.cuda.device(DEV):
        ctx = torch.empty(B, C, ld, device=DEV)
        n = int(lib.mvn_upsample_features_scratch_floats(B, C, F))
        scratch = torch.empty(n, device=DEV)
        N.check(lib.mvn_upsample_features_win(mel.data_ptr(), F, w.data_ptr(), bias.data_ptr(), B, M, F, C, taps, hop, T,
                                              ctx.data_ptr(), ld, scratch.data_ptr(), n, _stream()), "upsample")
        tm = torch.empty(B, T, C, device=DEV)
        N.check(lib.mvn_transpose_context(ctx.data_ptr(), ld, B, C, T, tm.data_ptr(), _stream()), "transpose")
        tm_g = tm.clone()
        N.check(lib.mvn_context_add_global(tm_g.data_ptr(), glob.data_ptr(), B, C, T, 0, _stream()), "add_global")
        glob2 = torch.cat([torch.zeros_like(glob), glob], 0).contiguous()
        tm_2g = torch.cat([tm, tm], 0).contiguous()
        N.check(lib.mvn_context_add_global(tm_2g.data_ptr(), glob2.data_ptr(), 2 * B, C, T, 0, _stream()), "add_global")
        filled = torch.empty(B, T, C, device=DEV)
        N.check(lib.mvn_context_add_global(filled.data_ptr(), glob.data_ptr(), B, C, T, 1, _stream()), "fill")
    torch.cuda.synchronize()
    return dict(mel=mel, w=w, bias=bias, glob=glob, glob2=glob2, F=F, proj=scratch[:B * C * F].view(B, C, F).clone(),
                tm=tm, tm_g=tm_g, tm_2g=tm_2g, filled=filled)


def _window_in_bands(rows, C, offset=0, **kw):
    """ops.context_window into the middle of a sentinel-filled allocation; returns (window, the two bands)."""
    n = kw["n"]
    count = rows * n * C
    raw = torch.full((2 * BAND + count + 4,), SENTINEL, device=DEV)
    assert raw.data_ptr() % 16 == 0
    lo = BAND + offset
    out = ops.context_window(out=raw[lo:lo + count], **kw)
    assert tuple(out.shape) == (rows, n, C) and out.data_ptr() == raw[lo:].data_ptr()
    return out, raw[:lo], raw[lo + count:]


WINDOWS = [(0, 1), (6, 2), (5, 1000), (T - 9, 9), (0, T)]


@pytest.mark.parametrize("taps", [1, 5])
@pytest.mark.parametrize("hop", [7, 256])
@pytest.mark.parametrize("C", [16, 64, 128])
def test_window_is_todays_three_kernel_path_bit_for_bit(C, hop, taps):
    ref = _reference(C, hop, taps)
    F = ref["F"]
    assert F == {7: 158, 256: 5}[hop]
    with torch.cuda.device(DEV):
        proj = torch.full((B, C, F + 3), SENTINEL, device=DEV)  # (a row stride above the frame count)
        N.check(N.lib().mvn_project_features(ref["mel"].data_ptr(), F, ref["w"].data_ptr(), ref["bias"].data_ptr(), B, M,
                                             F, C, taps, proj.data_ptr(), F + 3, _stream()), "mvn_project_features")
    assert torch.equal(_bits(proj[:, :, :F]), _bits(ref["proj"])), "mvn_project_features differs from the up-sampler's scratch"
    assert bool((proj[:, :, F:] == SENTINEL).all())
    proj = proj[:, :, :F]  # (batch, C, F) with rows F + 3 apart: the wrapper passes the stride on
    for t0, n in WINDOWS:
        cases = (("no label", dict(proj=proj), B, ref["tm"]),
                 ("label", dict(proj=proj, glob=ref["glob"]), B, ref["tm_g"]),
                 ("label alone", dict(proj=None, glob=ref["glob"]), B, ref["filled"]),
                 ("pairs", dict(proj=proj, glob=ref["glob2"], proj_rows=B), 2 * B, ref["tm_2g"]))
        for name, kw, rows, want in cases:
            got, front, back = _window_in_bands(rows, C, hop=hop, t0=t0, n=n, **kw)
            torch.cuda.synchronize()
            where = (C, hop, taps, t0, n, name)
            assert torch.equal(_bits(got), _bits(want[:, t0:t0 + n, :])), where
            assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), where
    assert not torch.equal(ref["tm"], ref["tm_g"])  # the label's vector was in force


@pytest.mark.parametrize("C,offset", [(16, 1), (64, 3), (6, 0), (7, 2)])
def test_one_channel_per_store_where_sixteen_bytes_do_not_fit(C, offset):
    """A window that does not start on 16 bytes, or whose channel count is no multiple of 4, takes the kernel's
    one-word stores: the same bits, the same bands."""
    hop, taps = 7, 5
    if C in (16, 64):
        ref = _reference(C, hop, taps)
        proj, glob, want = ref["proj"], ref["glob"], ref["tm_g"]
    else:  # (no reference of today's path needed: the 16-byte form of the same kernel is pinned above)
        g = torch.Generator().manual_seed(C)
        F = (T - 1) // hop + 1
        p4 = torch.randn(B, 8, F, generator=g).to(DEV)
        g4 = torch.randn(B, 8, generator=g).to(DEV)
        want = ops.context_window(p4, hop, 0, T, glob=g4)[:, :, :C].contiguous()
        proj, glob = p4[:, :C].contiguous(), g4[:, :C].contiguous()
    for t0, n in ((5, 1000), (T - 9, 9)):
        got, front, back = _window_in_bands(B, C, offset=offset, proj=proj, hop=hop, t0=t0, n=n, glob=glob)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want[:, t0:t0 + n, :])), (C, offset, t0, n)
        assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all())


def test_wrapper_checks():
    ref = _reference(16, 7, 1)
    with pytest.raises(ValueError, match="both None"):
        ops.context_window(None, 7, 0, 4)
    with pytest.raises(ValueError, match="too few frames"):
        ops.context_window(ref["proj"], 7, T, 7)   # 158 frames reach column 1105
    with pytest.raises(ValueError, match="glob must be"):
        ops.context_window(ref["proj"], 7, 0, 4, glob=ref["glob"][:, :8])
    with pytest.raises(ValueError, match="out must be"):
        ops.context_window(ref["proj"], 7, 0, 4, out=torch.empty(10, device=DEV))
    # the last column the frames reach: 157 * 7 + 6
    assert tuple(ops.context_window(ref["proj"], 7, 1105, 1).shape) == (B, 1, 16)
