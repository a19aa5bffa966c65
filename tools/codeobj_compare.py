#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libstark_hip.so, object file by object file.

    python tools/codeobj_compare.py PARENT_OBJ_DIR BRANCH_OBJ_DIR [--out profiles/NAME.json] [--brief]

For every *.o of both directories the gfx950 code object is taken out of the object's fat binary,
and for every kernel in it the compiler's metadata (VGPRs, SGPRs, scratch bytes, static LDS bytes) is
read with llvm-readelf and the instructions with llvm-objdump.  A kernel present in both builds is
"same" when the four figures, the instruction count and a hash of the instruction text (mnemonics and
operands, in order; addresses and encodings left out) all agree.  Needs no GPU.  The answer to "did
a change that adds instantiations in translation units of their own leave the existing kernels
alone" -- e.g. the Poisson family's sweep_pois.o / sweep16_pois.o / sweep16w_pois.o (-DSTK_SWEEP_TU=4).
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    fb = os.path.join(tmp, "x.hipfb")
    co = os.path.join(tmp, "x.co")
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--targets={TARGET}", f"--output={co}")
    return co


def kernels(obj):
    """{demangled kernel name: figures} of one object file."""
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", obj):
        return {}                      # host code only (capi.o)
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
        dis = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co)
    # a kernel's map has its keys in alphabetical order: .args (whose entries may carry a .name of
    # their own) come first, .group_segment_fixed_size opens the part read here, .wavefront_size ends it
    meta = {}
    cur = None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "group_segment_fixed_size":
            cur = {}
        if cur is None:
            continue
        cur[k] = v
        if k == "wavefront_size":
            meta[cur["name"]] = cur
            cur = None
    out = {}
    name, text = None, []

    def close():
        if name in meta:
            m = meta[name]
            out[name] = {"vgpr": int(m["vgpr_count"]), "sgpr": int(m["sgpr_count"]),
                         "scratch_bytes": int(m["private_segment_fixed_size"]),
                         "lds_static_bytes": int(m["group_segment_fixed_size"]),
                         "vgpr_spills": int(m.get("vgpr_spill_count", 0)), "sgpr_spills": int(m.get("sgpr_spill_count", 0)),
                         "instructions": len(text), "text_sha1": hashlib.sha1("\n".join(text).encode()).hexdigest()[:16]}

    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            close()
            name, text = m.group(1), []
            continue
        if line.startswith("\t") and name:
            text.append(re.sub(r"\s*//.*$", "", line).strip())
    close()
    names = list(out)
    if names and shutil.which("c++filt"):      # readable names where a demangler is installed
        dem = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
        out = {d: out[n] for d, n in zip(dem, names)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--out")
    ap.add_argument("--brief", action="store_true", help="record counts of unchanged kernels and one line per changed one")
    ap.add_argument("--parent-label", default="parent commit")
    ap.add_argument("--branch-label", default="this change")
    a = ap.parse_args()
    res = {"what": "gfx950 kernels of two builds of libstark_hip.so, per object file: VGPRs, SGPRs, scratch bytes, "
                   "static LDS bytes, spills, instruction count and a hash of the instruction text; 'same' = all equal",
           "parent": a.parent_label, "branch": a.branch_label, "objects": {}}
    objs = sorted({f for d in (a.parent, a.branch) for f in os.listdir(d) if f.endswith(".o")})
    nsame = ndiff = nnew = ngone = 0
    for o in objs:
        pa, br = os.path.join(a.parent, o), os.path.join(a.branch, o)
        kp = kernels(pa) if os.path.exists(pa) else {}
        kb = kernels(br) if os.path.exists(br) else {}
        same = sorted(k for k in kp if k in kb and kp[k] == kb[k])
        changed = {k: {"parent": kp[k], "branch": kb[k]} for k in kp if k in kb and kp[k] != kb[k]}
        new = {k: kb[k] for k in kb if k not in kp}
        gone = sorted(k for k in kp if k not in kb)
        nsame, ndiff, nnew, ngone = nsame + len(same), ndiff + len(changed), nnew + len(new), ngone + len(gone)
        res["objects"][o] = {"same": {k: kb[k] for k in same}, "changed": changed, "new": new, "gone": gone}
    res["summary"] = {"kernels_same": nsame, "kernels_changed": ndiff, "kernels_new": nnew, "kernels_gone": ngone}
    if a.brief:
        keys = ("vgpr", "sgpr", "scratch_bytes", "lds_static_bytes", "vgpr_spills", "sgpr_spills", "instructions")
        res["brief"] = "same: a count; changed: 'parent>branch' of " + ", ".join(keys) + "; new: those figures per kernel"
        for r in res["objects"].values():
            r["same"] = len(r["same"])
            r["changed"] = {k: " ".join(f"{v['parent'][f]}>{v['branch'][f]}" for f in keys) for k, v in r["changed"].items()}
            r["new"] = {k: " ".join(f"{f}={v[f]}" for f in keys) for k, v in sorted(r["new"].items())}
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res["summary"]))
    for o, r in res["objects"].items():
        for k in r["changed"]:
            print("CHANGED", o, k)
    return 1 if ndiff or ngone else 0


if __name__ == "__main__":
    sys.exit(main())
