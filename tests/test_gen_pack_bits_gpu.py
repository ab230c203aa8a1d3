"""GPU: mvn_gen_pack_weights writes, for every generator variant, the bytes it wrote BEFORE the packers moved behind
the variant descriptors (csrc/gen_common.h: GenVariant.pack, one contract for the context section in all five).

The deterministic synthetic weights (make_state_dict, seed 1) are packed with and without the context convs, each
variant at the smallest dims it accepts; the packed tensor is filled with a sentinel first, so the bytes a pack never
writes (the whole context section of a model without context convs, the slack behind PIPE_F16's half-size one) are
part of the SHA-256, and a pack that writes short of a section, past it or into the wrong one changes the hash.  A
band of sentinels in front of and behind the tensor catches a write outside it.  The hashes were recorded on an MI355X
from the library as it was before the change (tests/golden/gen_pack_sha256.json).

The fixture is only worth something recorded from a library built at the commit BEFORE the descriptors: --record
refuses to run unless MOVENET_HIP_LIB names the library it is to record from.

    MOVENET_HIP_LIB=<library built at that commit> python tests/test_gen_pack_bits_gpu.py --record
"""
import hashlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import DEV, SENTINEL, _Guard
from movenet_amd import _native as N
from movenet_amd.generation import pack_params
from movenet_amd.utils.weights import make_state_dict

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_pack_sha256.json")

SMALL = dict(layer_size=2, stack_size=2, input_channels=64, residual_channels=64, skip_channels=64)
WIDE = dict(layer_size=2, stack_size=2, input_channels=256, residual_channels=128, skip_channels=128)
CASES = [(name, variant, cfg, ctx)
         for name, variant, cfg in (("GENERIC", N.GEN_GENERIC, SMALL), ("STREAM", N.GEN_STREAM, SMALL),
                                    ("PIPE", N.GEN_PIPE, SMALL), ("FOLD", N.GEN_FOLD, SMALL),
                                    ("PIPE", N.GEN_PIPE, WIDE), ("PIPE_F16", N.GEN_PIPE_F16, WIDE))
         for ctx in (False, True)]


def case_id(name, cfg, ctx):
    return f"{name}-C{cfg['residual_channels']}-Q{cfg['input_channels']}-{'ctx' if ctx else 'noctx'}"


def packed_sha256(variant, cfg, ctx):
    lib = N.lib()
    sd = make_state_dict(**cfg, seed=1)
    if not ctx:
        sd = {k: v for k, v in sd.items() if "context_conv" not in k}
    sd = {k: v.to(DEV) for k, v in sd.items()}
    dims = N.make_dims(**cfg)
    guard = _Guard(front=True)
    with torch.cuda.device(DEV):
        packed = guard.new((lib.mvn_gen_weights_floats(dims, variant),), fill=SENTINEL, name="packed weights")
        params, keep = pack_params(dims, sd, cfg["layer_size"] * cfg["stack_size"])
        N.check(lib.mvn_gen_pack_weights(dims, variant, params, packed.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "mvn_gen_pack_weights")
    guard.check("mvn_gen_pack_weights")  # (synchronises)
    del keep
    return hashlib.sha256(packed.cpu().numpy().tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant,cfg,ctx", CASES, ids=[case_id(n, c, x) for n, _, c, x in CASES])
def test_packed_bytes_equal_the_recording(name, variant, cfg, ctx):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert packed_sha256(variant, cfg, ctx) == want[case_id(name, cfg, ctx)]


if __name__ == "__main__":
    assert "--record" in sys.argv and os.environ.get("MOVENET_HIP_LIB"), __doc__
    out = {case_id(n, c, x): packed_sha256(v, c, x) for n, v, c, x in CASES}
    assert len(out) == len(CASES)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))
