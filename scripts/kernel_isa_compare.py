#!/usr/bin/env python3
"""Compare kernels of two builds by their assembly text.

    python scripts/kernel_isa_compare.py PARENT_LIB BRANCH_LIB [--out=profiles/layer_kernel_scaffold.json] [--dump=DIR]

--out=FILE merges the result into that JSON file; --dump=DIR writes the normalised text of every kernel that differs
to DIR/<kernel>.parent.s and DIR/<kernel>.branch.s, to be diffed.

Each LIB is a movenet_amd/lib directory left by `python -m movenet_amd.csrc.build --force --keep-temps` (or the
sequence-hip-amdgcn-amd-amdhsa-gfx950.s file itself).  For each layer kernel (KERNELS) and each instantiation of the
PREFIXES' templates that the file holds: the resource figures the compiler prints behind the kernel (the ones -Rpass-analysis=kernel-resource-usage reports), the code bytes, and the
SHA-256 of the instruction text from the kernel's label to its s_endpgm with comments stripped and local labels
renumbered.  Text only: no instruction is looked for.  The kernels of REPORTED (and REPORTED_PREFIXES) -- the weight
pack kernels, which run once per forward call -- are listed with the same figures under "reported"; they do not decide
the exit status.
"""
import hashlib
import json
import os
import re
import sys

ASM = "sequence-hip-amdgcn-amd-amdhsa-gfx950.s"
KERNELS = [
    "bwd_layer64_kernel<false>", "bwd_layer64_kernel<true>",
    "bwd_layer64_bf16_kernel<false, false>", "bwd_layer64_bf16_kernel<true, false>", "bwd_layer64_bf16_kernel<false, true>",
    "fused_layer64s_bf3_kernel<false>", "fused_layer64s_bf3_kernel<true>",
    "fused_layer64s_bf16_kernel<false, false>", "fused_layer64s_bf16_kernel<true, false>",
    "fused_layer64s_bf16_kernel<false, true>",
    "fused_layer64s_kernel<false>", "fused_layer64s_kernel<true>", "fused_layer64s_ctxw2_kernel",
    "bwd_dz_wgrs64_kernel", "bwd_dctx_wgctx64_kernel", "bwd_dx_wgfg64_kernel",
]
PREFIXES = ["dense_strip_bf3_kernel<"]  # every instantiation sequence.hip emits
REPORTED = ["fs3_pack_kernel", "fb16_pack_kernel", "fb16c_pack_kernel", "fsc_pack_kernel"]
REPORTED_PREFIXES = ["ds3_pack_kernel<"]
FIGURES = {"vgpr": "NumVgprs", "agpr": "NumAgprs", "sgpr": "TotalNumSgprs", "scratch_bytes": "ScratchSize",
           "lds_bytes": "LDSByteSize", "occupancy": "Occupancy", "code_bytes": "codeLenInByte"}


def short_name(sym):
    """_ZN3mvn18bwd_layer64_kernelILb1EEEv... -> bwd_layer64_kernel<true>; ...kernelILi64ELb0EEEv -> kernel<64, false>;
    _ZN3mvn27fused_layer64s_ctxw2_kernelENS_... (no template) -> fused_layer64s_ctxw2_kernel"""
    m = re.match(r"_ZN3mvn\d+([a-z0-9_]+?)(?:I((?:L[bi]\d+E)+)E|E)", sym)
    if not m:
        return sym
    if not m.group(2):
        return m.group(1)
    args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([bi])(\d+)E", m.group(2))]
    return "%s<%s>" % (m.group(1), ", ".join(args))


def wanted(name, names, prefixes):
    return name in names or any(name.startswith(p) for p in prefixes)


def kernels_of(path):
    if os.path.isdir(path):
        path = os.path.join(path, ASM)
    lines = open(path).read().split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m]
    short = {s: short_name(s) for _, s in starts}
    res = {}
    for n, (i, sym) in enumerate(starts):
        if not wanted(short[sym], KERNELS + REPORTED, PREFIXES + REPORTED_PREFIXES):
            continue
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        body, tail = [], lines[i:end]
        for j, l in enumerate(tail):
            code = l.split(";")[0].rstrip()
            if code.strip():
                body.append(code)
            if code.strip() == "s_endpgm":
                tail = tail[j:]
                break
        labels = {}
        text = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(body))
        text = text.replace(sym, "KERNEL")
        rec = {"sha256": hashlib.sha256(text.encode()).hexdigest(), "lines": len(body)}
        for key, word in FIGURES.items():
            m = re.search(r";\s*%s\s*[:=]\s*(\d+)" % word, "\n".join(tail))
            rec[key] = int(m.group(1)) if m else None
        res[short[sym]] = (rec, text)
    return res


# The kernels' LDS is dynamic, so the compiler reports 0 bytes: what their launchers pass instead (the constants of
# fused_bwd_l.h, fused_fwd_bf3.h and fused_bf16.h; the bias forms add GBIAS_LDS_BYTES = 512).  The two 256-thread passes
# of fused_bwd.h declare theirs statically: the compiler reports the same figure.  Unchanged by a refactor
# that leaves those constants alone; kept here so that the file this script writes says what a workgroup occupies.
LAUNCH_LDS_BYTES = {
    "bwd_layer64_kernel<false>": 153600, "bwd_layer64_kernel<true>": 153600,                      # FBL_LDS_BYTES
    "bwd_layer64_bf16_kernel<false, false>": 120832, "bwd_layer64_bf16_kernel<true, false>": 120832,
    "bwd_layer64_bf16_kernel<false, true>": 120832,                                               # FBL16_LDS_BYTES
    "fused_layer64s_bf3_kernel<false>": 147968, "fused_layer64s_bf3_kernel<true>": 148480,        # FS3_LDS_BYTES (+ 512)
    "fused_layer64s_bf16_kernel<false, false>": 49664, "fused_layer64s_bf16_kernel<true, false>": 50176,  # FB16_LDS_BYTES
    "fused_layer64s_bf16_kernel<false, true>": 66560,                                             # FB16C_LDS_BYTES
    "fused_layer64s_kernel<false>": 99328, "fused_layer64s_kernel<true>": 132096,                 # F32_STRIP(_CTX)_LDS_BYTES
    "fused_layer64s_ctxw2_kernel": 163840,                                                        # FSC_LDS_BYTES
    "bwd_dz_wgrs64_kernel": 69632, "bwd_dctx_wgctx64_kernel": 69632,            # static: (128 + 64 + 64) x W2_LD x 4
    "bwd_dx_wgfg64_kernel": 139264,                                                               # FBB_LDS_FLOATS x 4
}


def launch_lds_bytes(k):
    if k.startswith("dense_strip_bf3_kernel<"):  # <K, M, ...>: K x M x 6 bytes of planes + M floats of bias
        K, M = [int(v) for v in k[k.index("<") + 1:].split(", ")[:2]]
        return K * M * 6 + M * 4
    return LAUNCH_LDS_BYTES[k]


def option(name):
    """--name=VALUE or None"""
    return next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)), None)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out, dump = option("out"), option("dump")
    parent, branch = kernels_of(args[0]), kernels_of(args[1])
    doc = {"kernels": {}, "reported": {}}
    both = sorted(set(parent) | set(branch))
    for k in [k for k in both if wanted(k, REPORTED, REPORTED_PREFIXES)]:
        p, b = parent[k], branch[k]
        doc["reported"][k] = {"parent": p[0], "branch": b[0], "identical": p[1] == b[1]}
        print("%-45s %s  vgpr %s/%s sgpr %s/%s scratch %s/%s code %s/%s (reported only)" % (
            k, "same" if p[1] == b[1] else "differs", p[0]["vgpr"], b[0]["vgpr"], p[0]["sgpr"], b[0]["sgpr"],
            p[0]["scratch_bytes"], b[0]["scratch_bytes"], p[0]["code_bytes"], b[0]["code_bytes"]))
    for k in KERNELS + [k for k in both if wanted(k, [], PREFIXES)]:
        p, b = parent[k], branch[k]
        doc["kernels"][k] = {"parent": p[0], "branch": b[0], "identical": p[1] == b[1],
                             "launch_lds_bytes": launch_lds_bytes(k)}
        print("%-45s %s  vgpr %s/%s scratch %s/%s occ %s/%s" % (k, "same" if p[1] == b[1] else "DIFFERS", p[0]["vgpr"], b[0]["vgpr"],
              p[0]["scratch_bytes"], b[0]["scratch_bytes"], p[0]["occupancy"], b[0]["occupancy"]))
        if p[1] != b[1] and dump:
            for tag, t in (("parent", p[1]), ("branch", b[1])):
                open(os.path.join(dump, "%s.%s.s" % (re.sub(r"\W+", "_", k), tag)), "w").write(t)
    if out:
        old = json.load(open(out)) if os.path.exists(out) else {}
        old.update(doc)
        json.dump(old, open(out, "w"), indent=1)
        open(out, "a").write("\n")
    return 0 if all(v["identical"] for v in doc["kernels"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
