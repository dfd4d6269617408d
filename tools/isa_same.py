"""Are the gfx950 instructions of the kernels two builds share the same?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -fuse-cuid=none -o a.s ectrans_amd/csrc/ectrans_mi.hip   (each tree)
    python tools/isa_same.py parent.s branch.s

Compares the body of every function present in both assembly files after removing what depends on a function's position in the
file rather than on its code: the function number in local labels (.LBB12_3), comments, trailing blanks.  Prints the kernels that
differ and the ones only one side has; exit code 1 if a shared kernel differs."""
import re
import sys


def kernels(path):
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\s*\.size\s+\1,", open(path).read(), re.S | re.M):
        body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
        body = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", body)
        out[m.group(1)] = "\n".join(l.split(";")[0].rstrip() for l in body.split("\n"))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    shared = sorted(set(a) & set(b))
    diff = [k for k in shared if a[k] != b[k]]
    print("%d functions in %s, %d in %s, %d in both: %d identical, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], len(shared), len(shared) - len(diff), len(diff)))
    for k in diff:
        print("  differs:", k)
    for k in sorted(set(a) - set(b)):
        print("  only in the first: ", k)
    for k in sorted(set(b) - set(a)):
        print("  only in the second:", k)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
