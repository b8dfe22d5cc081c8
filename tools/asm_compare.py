"""Compare the device code of every kernel in two sets of hipcc -S listings (development tool):
   tools/asm_compare.py BASE_DIR NEW_DIR
Each directory holds the listings of the same sources (hipcc --cuda-device-only -S with the Makefile's flags).  For every kernel of
BASE_DIR, NEW_DIR must hold a kernel of the same mangled name with the same instructions (comments and block numbers dropped) and the
same kernel descriptor."""
import os
import re
import sys


def funcs(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.M | re.S):
        out[m.group(1)] = re.sub(r';.*', '', re.sub(r'\.LBB\d+_\d+|\.Ltmp\d+|BB\d+_\d+', 'L', m.group(2)))
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel', txt, re.M | re.S):
        out['KD:' + m.group(1)] = m.group(2)
    return out


def main(base, new):
    bad = tot = 0
    for f in sorted(os.listdir(base)):
        a, b = funcs(os.path.join(base, f)), funcs(os.path.join(new, f))
        missing = [k for k in a if k not in b]
        diff = [k for k in a if k in b and a[k] != b[k]]
        added = [k for k in b if k not in a]
        tot += len(a)
        bad += len(missing) + len(diff)
        print(f"{f:22s} functions+descriptors {len(a):3d}  identical {len(a) - len(missing) - len(diff):3d}  differ {len(diff)}  missing {len(missing)}  added {len(added)}")
        for k in diff + missing:
            print('   !!', k)
    print(f"compared {tot}, not identical {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
