"""Kernel-by-kernel comparison of two sets of assembly listings (make -C iv_interpolation_amd/csrc asm -> build/<unit>.s).
    python tools/asm_diff.py <before> [<after> [regex applied to the BEFORE names, replaced by ""]]
<before> / <after>: a listing, a directory (every *.s in it) or a comma-separated list of listings; <after> defaults to build/.
Bodies and kernel descriptors are compared with comments stripped and the function number taken out of local labels;
the optional regex removes a dropped template argument from the mangled names, e.g. '(?<=surface_dense_var_kernelILi\\dE)Li1E'
turns ...surface_dense_var_kernelILi0ELi1ELb1ELb1EE... into ...surface_dense_var_kernelILi0ELb1ELb1EE..."""
import glob, os, re, sys


def listings(arg):
    return [p for a in arg.split(",") for p in (sorted(glob.glob(os.path.join(a, "*.s"))) if os.path.isdir(a) else [a])]


def kernels(arg, drop):
    out = {}
    for path in listings(arg):
        for name, body in kernels_of(path, drop).items():
            assert name not in out, f"{name} is in two listings of {arg}"
            out[name] = body
    return out


def kernels_of(path, drop):
    t = open(path).read()
    out = {}
    for m in re.finditer(r"^(\S+): +; @", t, re.M):
        name = m.group(1)
        end = t.index(".Lfunc_end", m.end())
        desc = re.search(r"^\t\.amdhsa_kernel %s\n(.*?)^\t\.end_amdhsa_kernel" % re.escape(name), t[end:], re.M | re.S)
        text = t[m.end():end] + (desc.group(1) if desc else "")
        lines = [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in text.split("\n")]
        body = "\n".join(l for l in lines if l)
        body = re.sub(r"\.L(BB|tmp|func_begin)\d+_", r".L\1_", body).replace(name, "@self")
        out[re.sub(drop, "", name) if drop else name] = body
    return out


if len(sys.argv) not in (2, 3, 4):
    sys.exit(__doc__)
a, b = kernels(sys.argv[1], sys.argv[3] if len(sys.argv) > 3 else None), kernels(sys.argv[2] if len(sys.argv) > 2 else "build", None)
for n in sorted(set(a) ^ set(b)): print("only in", "before" if n in a else "after", n)
diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
for n in diff: print("differs", n, len(a[n].split("\n")), "->", len(b[n].split("\n")), "lines")
print(f"{len(a)} kernels before, {len(b)} after, {len(set(a) & set(b)) - len(diff)} identical, {len(diff)} differ")
