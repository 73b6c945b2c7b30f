"""Per-kernel comparison of two device assembly listings (`make asm` output) of
the same source file from two builds; needs no GPU (dev tool):

    python tools/isa_same.py PARENT.s NEW.s [out.json [PARENT.so NEW.so]]   # exit 1 on a difference

A listing is cut at its kernel symbols: from `.type <kernel>,@function` to the
kernel's `.Lfunc_end` (the `.amdhsa_kernel` descriptor lies in between).  Inside
a kernel its own mangled name is replaced by a placeholder and comments are
dropped, so a kernel whose template parameter list changed still compares equal
to its old self: kernels with no namesake in the other file are paired when they
share the base name and the text.  Two compiles of one source differ only in the
`__hip_cuid_*` symbol, which lies outside every kernel.  With the two libraries,
the report also carries the metadata resources (tests/helpers/codeobj.py) of the
kernels that differ and the waves per SIMD they allow."""
import json
import os
import re
import sys
import tempfile


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n", text, re.M):
        name = m.group(1)
        end = text.find(".Lfunc_end", m.end())
        end = text.find("\n", end)
        body = text[m.end():end].replace(name, "@KERNEL")
        body = re.sub(r"\s*;.*$", "", body, flags=re.M)   # comments (they number other functions)
        # local labels are numbered per file: .LBB<function index>_<block>
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
        out[name] = re.sub(r"\n+", "\n", body)
    return out


def base(name):
    m = re.search(r"\d+([A-Za-z_][A-Za-z0-9_]*?_kernel)", name)
    return m.group(1) if m else name


def targs(name):  # the integer template arguments in a mangled name
    return re.findall(r"Li(\d+)E", name.split("_kernel")[1].split("EEv")[0])


def resources(lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from helpers import codeobj
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for co in codeobj.extract(lib, d):
            for k, v in codeobj.kernel_resources(co).items():
                v["waves_per_simd"] = codeobj.waves_per_simd(v.get("vgpr", 0), v.get("agpr", 0))
                res[k] = v
    return res


def main(a_path, b_path, out_path=None, a_lib=None, b_lib=None):
    a, b = kernels(a_path), kernels(b_path)
    res, pair = {}, {}
    for n in sorted(set(a) & set(b)):
        res[n] = "identical" if a[n] == b[n] else "DIFFERENT"
        pair[n] = n
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for identical in (True, False):  # renamed kernels: equal text first, then what is left
        for nb in list(only_b):
            tb = targs(nb)
            cand = [na for na in only_a if base(na) == base(nb) and
                    (a[na] == b[nb] if identical else targs(na)[len(targs(na)) - len(tb):] == tb)]
            if cand:  # of several namesakes, the one nearest in length
                na = min(cand, key=lambda x: abs(len(a[x]) - len(b[nb])))
                res[nb] = ("identical (was %s)" if identical else "DIFFERENT (was %s)") % na
                pair[nb] = na
                only_a.remove(na)
                only_b.remove(nb)
    for n in only_a:
        res[n] = "removed"
    for n in only_b:
        res[n] = "NEW"
    bad = sorted(n for n, v in res.items() if v.startswith(("DIFFERENT", "NEW")))
    rep = {"file": os.path.basename(b_path), "kernels": res, "differing": bad}
    if a_lib and b_lib:
        ra, rb = resources(a_lib), resources(b_lib)
        rep["resources_of_differing"] = {n: {"parent": ra.get(pair.get(n, n)), "new": rb.get(n)}
                                         for n in bad}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps({"kernels": len(res), "removed": sum(v == "removed" for v in res.values()),
                      "differing": bad}))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:6]))
