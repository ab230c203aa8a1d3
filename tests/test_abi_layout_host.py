"""CPU: the struct layouts are the one mirror of include/movenet_hip.h that Python still writes out by hand -- the
ctypes Structure classes of movenet_amd/_native.py and the numpy record dtypes of the device-side descriptors in
movenet_amd/ops.py.  A host-only C program that includes the header prints sizeof and every field's offsetof; both
mirrors must agree with it.  (A field the header does not have fails the compile.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from movenet_amd import _native as N
from movenet_amd import ops
from movenet_amd.csrc import build

STRUCTURES = {"mvn_dims": N.Dims, "mvn_params": N.Params, "mvn_param_grads": N.ParamGrads,
              "mvn_fwd_buffers": N.FwdBuffers, "mvn_bwd_buffers": N.BwdBuffers, "mvn_seq_sampling": N.SeqSampling,
              "mvn_video_params": N.VideoParams, "mvn_video_grads": N.VideoParams,
              "mvn_block_tensor": N.BlockTensor, "mvn_block_gated_params": N.BlockGatedParams,
              "mvn_block_gated_grads": N.BlockGatedParams}
DESCRIPTORS = {"mvn_audio_clip": ops._AUDIO_CLIP, "mvn_audio_clip_var": ops._AUDIO_CLIP_VAR,
               "mvn_audio_clip_window": ops._AUDIO_CLIP_WINDOW, "mvn_video_clip": ops._VIDEO_CLIP}


def _python_layouts():
    """{C type: (size, {field: (offset, size)})} as the two Python mirrors have it."""
    out = {}
    for name, cls in STRUCTURES.items():
        out[name] = (C.sizeof(cls), {f: (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
    for name, fields in DESCRIPTORS.items():
        dtype = np.dtype(fields)
        out[name] = (dtype.itemsize, {f: (dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names})
    return out


def test_struct_layouts_are_the_headers(tmp_path):
    try:
        compiler = build._hipcc()
    except RuntimeError as e:
        pytest.skip(f"no compiler: {e}")
    want = _python_layouts()
    assert len(STRUCTURES) == 11 and len({id(c) for c in STRUCTURES.values()}) == 9 and len(DESCRIPTORS) == 4
    lines = ['#include <stdio.h>', '#include "movenet_hip.h"', "int main(void) {"]
    for name, (_, fields) in want.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for f in fields:
            lines.append(f'  printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    # host compilation only: plain C, no offload arch, nothing of the GPU runtime
    cc = subprocess.run([compiler, "-x", "c", "-std=c11", "-I", os.path.dirname(N.HEADER_PATH), str(src),
                         "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = {}
    for key, *numbers in (line.split() for line in run.stdout.splitlines()):
        got[key] = tuple(int(n) for n in numbers)
    for name, (size, fields) in want.items():
        assert got[name] == (size,), f"sizeof({name}): the header has {got[name][0]}, Python {size}"
        for f, layout in fields.items():
            assert got[f"{name}.{f}"] == layout, f"{name}.{f}: (offset, size) {got[name + '.' + f]} in the header, " \
                                                 f"{layout} in Python"
        # the fields tile the struct: no member of the header is missing between or behind them but alignment padding
        end = max(o + s for o, s in fields.values())
        assert size - end < 8, f"{name}: {size - end} bytes behind the last field Python knows"
    assert len(got) == sum(1 + len(fields) for _, fields in want.values())
