"""Compare two device-only assembly builds (hipcc --cuda-device-only -S) kernel by kernel.

usage: python scripts/isa_same.py A.s B.s
Per mangled kernel name: the instructions and the .amdhsa_kernel descriptor, without comments and debug
directives and with the label numbers replaced.  Prints the kernels only one file has and those whose
text differs; exit status 1 if a kernel that both have differs.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
        body = re.search(rf"^{re.escape(name)}:.*?^\.Lfunc_end\d+:", text, re.M | re.S).group(0)
        desc = re.search(rf"^\s*\.amdhsa_kernel {re.escape(name)}$.*?\.end_amdhsa_kernel", text, re.M | re.S).group(0)
        lines = []
        for ln in (body + "\n" + desc).splitlines():
            ln = re.sub(r"\.(LBB\d+_\d+|Ltmp\d+|Lfunc_end\d+|Lfunc_begin\d+)", ".L", ln.split(";")[0]).strip()
            if ln and not re.match(r"\.(loc|file|cfi_\w+)\b", ln):
                lines.append(ln)
        out[name] = lines
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = [k for k in a if k in b and a[k] != b[k]]
    for k in a:
        if k not in b:
            print("only in A:", k)
    for k in b:
        if k not in a:
            print("only in B:", k)
    for k in diff:
        print(f"differs: {k} ({len(a[k])} lines in A, {len(b[k])} in B)")
    print(f"{len(a)} kernels in A, {len(b)} in B, {sum(k in b for k in a) - len(diff)} identical, {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
