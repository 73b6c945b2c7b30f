"""Registers, LDS, scratch and waves per SIMD of every norm.hip kernel and every
gather_rows* instantiation, one library against another (CPU only; dev tool):

    python tools/norm_resources.py PARENT.so NEW.so [--out profiles/norm_core_resources.json]

A kernel of NEW is listed against the kernel of PARENT it replaces (RENAMED
below; the same demangled name otherwise; c++filt or llvm-cxxfilt demangles).
Exit status 1 when a kernel gains scratch, uses more LDS or drops a wave per
SIMD."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import codeobj as C  # noqa: E402

NORM = re.compile(r"\b(bn_\w+|gn_\w+|rowpart_sum)_kernel\b")
GATHER = re.compile(r"\bgather_rows\d?_kernel\b")
ANON = "pcfm::(anonymous namespace)::"
# new kernel -> the parent's kernel it replaces
RENAMED = {
    "bn_act_apply_kernel<(BnSink)0>": "bn_act_apply_kernel",
    "bn_act_apply_kernel<(BnSink)1>": "bn_act_rowsum_kernel",
    "bn_bwd_apply_split_kernel<BnPartSums>": "bn_bwd_apply_split_kernel",
    "bn_bwd_apply_split_kernel<BnSeSums>": "bn_se_bwd_apply_split_kernel",
}


def table(lib):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in C.extract(lib, d):
            res = C.kernel_resources(co)
            names = list(res)
            filt = shutil.which("c++filt") or C.tool("llvm-cxxfilt")
            dem = subprocess.run([filt] + names, capture_output=True, text=True,
                                 check=True).stdout.splitlines()
            for name, full in zip(names, dem):
                if not (NORM.search(full) or GATHER.search(full)):
                    continue
                # the template name without return type, namespaces and parameter list
                key = full.replace("void ", "").replace(ANON, "").replace("pcfm::", "")
                depth = 0  # the parameter list opens at the first "(" outside <...>
                for i, ch in enumerate(key):
                    depth += (ch == "<") - (ch == ">")
                    if ch == "(" and depth == 0:
                        key = key[:i]
                        break
                reg = C.descriptor_registers(co, name)
                r = res[name]
                out[key] = {"regs_alloc": reg["alloc"], "lds_bytes": r.get("lds", 0),
                            "scratch_bytes": r.get("scratch", 0),
                            "waves_per_simd": min(8, 512 // reg["alloc"])}
    return out


def main():
    parent, new = table(sys.argv[1]), table(sys.argv[2])
    rows, bad = [], []
    for key in sorted(new):
        pkey = RENAMED.get(key, key)
        p, n = parent.get(pkey), new[key]
        row = {"kernel": key, "replaces": pkey, "parent": p, "new": n}
        if p is None:
            row["violates"] = ["no parent kernel"]
        else:
            row["violates"] = [w for w, hit in (
                ("scratch", n["scratch_bytes"] > p["scratch_bytes"]),
                ("lds", n["lds_bytes"] > p["lds_bytes"]),
                ("waves", n["waves_per_simd"] < p["waves_per_simd"])) if hit]
        if row["violates"]:
            bad.append(key)
        rows.append(row)
    used = {r["replaces"] for r in rows}
    doc = {"conditions": "no kernel gains scratch, uses more LDS or drops a wave per SIMD",
           "parent_only": sorted(set(parent) - used), "violations": bad, "kernels": rows}
    text = json.dumps(doc, indent=1)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    for r in rows:
        p, n = r["parent"] or {}, r["new"]
        print(f"{r['kernel'][:78]:78s} regs {p.get('regs_alloc')}->{n['regs_alloc']} "
              f"lds {p.get('lds_bytes')}->{n['lds_bytes']} scratch {p.get('scratch_bytes')}->"
              f"{n['scratch_bytes']} waves {p.get('waves_per_simd')}->{n['waves_per_simd']} "
              f"{' '.join(r['violates'])}")
    print("parent only:", doc["parent_only"])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
