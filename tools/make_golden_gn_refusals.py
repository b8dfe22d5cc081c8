"""The refusals of the GroupNorm stage's C entry points, whole: return code and message of every refused call (CPU only).

    SGR_LIB=<libsgrender.so of the commit to pin> python tools/make_golden_gn_refusals.py      # writes tests/golden/gn_entry_refusals.json

Every one of the 13 launching entry points of csrc/sgr_gn_stage.hip (sgr_gn_stage_fwd / _bwd and their _bf16 forms, sgr_gn_resize_fwd /
_bwd, sgr_gn_moments, the four sgr_gn_{stage,resize}_siblings_* pairs counting bf16) is called from a baseline it would accept, with one
argument wrong at a time -- every distinct SGR_REQUIRE / SGR_SUPPORTED in it -- and with a few pairs of faults per family, which pin the
order of the checks: the message of the earlier check wins.  The device pointers are fake non-NULL addresses that no refused call
dereferences (tests/test_gn_stage.py::test_c_abi_refusals_without_gpu); the pointer tables and stride arrays of the sibling forms are
real host arrays, which the entry points read.  The four workspace queries are called on inputs for which they return 0.

tests/test_gn_entry_refusals.py imports CASES and call() from here and replays the file.  A change of the host code regenerates nothing:
the file is made once from the commit BEFORE a refactoring of the entry points and then holds them to it."""
from __future__ import annotations

import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gn_entry_refusals.json")

FAKE = 4096           # on every boundary the entry points test
ODD = FAKE + 4        # a float pointer that is not 8-byte aligned
MAXD = 8              # SGR_GN_MAX_SIBLINGS: the tables are always this long
NEG = (120, 15, -5, 1)
FAR = (120, 15, 1 << 31, 1)      # (H - 1) * stride_h does not fit 31 bits

SIZES = ["B", "C", "G", "Cs", "H", "W"]
RSIZES = SIZES + ["Hs", "Ws"]
TABLES = ("gs", "xs", "weights", "biases", "outs", "dxs", "dweights", "dbiases")


def _fwd(sizes):
    return ["x", "weight", "bias", "skip", "out", "stats", "workspace"] + sizes + ["x_strides", "skip_strides", "eps", "stream"]


def _bwd(sizes):
    return ["g", "x", "weight", "bias", "stats", "dx", "dweight", "dbias", "dskip", "workspace"] + sizes + ["x_strides", "stream"]


def _sfwd(sizes):
    return ["D", "xs", "weights", "biases", "skip", "outs", "stats", "workspace"] + sizes + ["x_strides", "skip_strides", "eps", "stream"]


def _sbwd(sizes):
    return ["D", "gs", "xs", "weights", "biases", "stats", "dxs", "dweights", "dbiases", "dskip", "workspace"] + sizes + ["x_strides", "stream"]


# entry point -> its arguments in order (include/sgrender.h)
ENTRIES = {
    "sgr_gn_stage_fwd": _fwd(SIZES), "sgr_gn_stage_bwd": _bwd(SIZES),
    "sgr_gn_stage_fwd_bf16": _fwd(SIZES), "sgr_gn_stage_bwd_bf16": _bwd(SIZES),
    "sgr_gn_resize_fwd": _fwd(RSIZES), "sgr_gn_resize_bwd": _bwd(RSIZES),
    "sgr_gn_moments": ["x", "stats", "workspace", "B", "C", "G", "H", "W", "x_strides", "eps", "stream"],
    "sgr_gn_stage_siblings_fwd": _sfwd(SIZES), "sgr_gn_stage_siblings_bwd": _sbwd(SIZES),
    "sgr_gn_stage_siblings_fwd_bf16": _sfwd(SIZES), "sgr_gn_stage_siblings_bwd_bf16": _sbwd(SIZES),
    "sgr_gn_resize_siblings_fwd": _sfwd(RSIZES), "sgr_gn_resize_siblings_bwd": _sbwd(RSIZES),
}
QUERIES = {
    "sgr_gn_stage_workspace_floats": ["B", "C", "G", "H", "W", "upcat", "backward"],
    "sgr_gn_resize_workspace_floats": ["B", "C", "G", "H", "W", "Hs", "Ws", "upcat", "backward"],
    "sgr_gn_stage_siblings_workspace_floats": ["D", "B", "C", "G", "H", "W", "backward"],
    "sgr_gn_resize_siblings_workspace_floats": ["D", "B", "C", "G", "H", "W", "Hs", "Ws", "backward"],
}
BASE = dict(D=2, B=2, C=8, G=2, Cs=4, H=3, W=5, Hs=5, Ws=7, eps=1e-5, stream=None, upcat=1, backward=1)


WORDS = {None: "NULL", ODD: "unaligned", NEG: "negative", FAR: "far"}


def label(fault):
    return ", ".join(f"{k}={WORDS.get(v, v)}" for k, v in fault.items())


def call(lib, entry, fault):
    """Call `entry` from the accepted baseline with the arguments of `fault` replaced.  Keys: an argument's name; `name[d]` for one entry
    of a pointer table; `x_strides[d]` for the strides of sibling d.  Returns (code, message)."""
    resize = "resize" in entry
    sib = "siblings" in entry
    names = ENTRIES.get(entry) or QUERIES[entry]
    a = dict(BASE)
    sh, sw = (a["Hs"], a["Ws"]) if resize else (a["H"], a["W"])
    strides = {"x_strides": [(120, 15, 5, 1)] * (MAXD if sib else 1), "skip_strides": [(a["Cs"] * sh * sw, sh * sw, sw, 1)]}
    tables = {t: [FAKE] * MAXD for t in TABLES}
    for k, v in fault.items():
        if "[" in k:
            name, d = k[:-1].split("[")
            (strides if name in strides else tables)[name][int(d)] = v
        else:
            a[k] = v
    keep = []      # the host arrays live until the call returns
    args = []
    for n in names:
        if n in a:
            v = a[n]
        elif n in strides:
            v = (ctypes.c_longlong * (4 * len(strides[n])))(*[s for four in strides[n] for s in four])
        elif n in tables:
            v = (ctypes.c_void_p * MAXD)(*tables[n])
        else:
            v = FAKE
        if isinstance(v, tuple):      # a whole stride array replaced
            v = (ctypes.c_longlong * (4 * MAXD))(*(list(v) * MAXD))
        keep.append(v)
        args.append(ctypes.c_float(v) if n == "eps" else v)
    code = getattr(lib, entry)(*args)
    if entry in QUERIES:
        return int(code), ""
    msg = (lib.sgr_last_error() or b"").decode()
    return int(code), msg.split(" [a HIP error was already pending")[0]


def _sizes(resize, sib, backward):
    out = [{k: bad} for k in ("B", "C", "G", "H", "W") for bad in (0, -3)]
    out += [{"G": 3}, {"B": 65536}, {"C": 65535, "G": 1}, {"H": 8192, "W": 8192}]
    if sib:
        out += [{"D": 0}, {"D": 9}, {"Cs": 0}, {"C": 32766}]      # D * C + Cs = 65536
    elif not backward:
        out += [{"Cs": -1}]
    if resize:
        out += [{"Hs": 0}, {"Ws": -1}, {"Hs": 2}, {"Hs": 7}, {"Ws": 4}, {"Ws": 11}, {"H": 8191, "W": 8191, "Hs": 8192, "Ws": 8192}]
    return out


def _cases():
    cases = []
    for entry in ENTRIES:
        resize, sib, backward = "resize" in entry, "siblings" in entry, "_bwd" in entry
        c = []
        if entry == "sgr_gn_moments":
            c += [{k: None} for k in ("x", "stats", "workspace", "x_strides")]
            c += [f for f in _sizes(False, False, False) if "Cs" not in f and f != {"C": 65535, "G": 1}] + [{"C": 65536, "G": 1}]
            c += [{"eps": 0.0}, {"eps": -1.0}, {"x_strides": NEG}, {"x_strides": FAR}, {"workspace": ODD}]
            c += [{"x": None, "B": 0}, {"B": 0, "eps": 0.0}, {"G": 3, "B": 65536}, {"eps": 0.0, "x_strides": NEG}, {"x_strides": NEG, "workspace": ODD}]
        elif not sib and not backward:
            c += [{k: None} for k in ("x", "weight", "bias", "out", "stats", "workspace", "x_strides")]
            c += [{"skip": None}, {"Cs": 0}, {"skip_strides": None}]
            c += _sizes(resize, False, False)
            c += [{"eps": 0.0}, {"eps": -1.0}, {"x_strides": NEG}, {"x_strides": FAR}, {"skip_strides": NEG}, {"workspace": ODD}]
            c += [{"x": None, "skip": None}, {"skip": None, "B": 0}, {"x": None, "B": 0}, {"B": 0, "eps": 0.0}, {"G": 3, "B": 65536},
                  {"B": 65536, "H": 8192, "W": 8192}, {"eps": 0.0, "x_strides": NEG}, {"x_strides": NEG, "workspace": ODD}]
            if resize:
                c += [{"B": 0, "Hs": 0}, {"H": 8192, "W": 8192, "Hs": 0}, {"Hs": 0, "Ws": 11}, {"Hs": 7, "eps": 0.0}]
        elif not sib:
            c += [{"g": None}, {"dx": None, "dweight": None, "dbias": None, "dskip": None}]
            c += [{k: None} for k in ("x", "weight", "bias", "stats", "workspace", "x_strides")]
            c += [{"Cs": 0}, {"dx": None, "dweight": None, "dbias": None, "Cs": 0}]
            c += _sizes(resize, False, True)
            c += [{"dx": None, "dweight": None, "dbias": None, "B": 0}]      # the skip's gradient alone: the sizes are still checked
            c += [{"workspace": ODD}, {"x_strides": NEG}, {"x_strides": FAR}]
            c += [{"g": None, "dx": None, "dweight": None, "dbias": None, "dskip": None}, {"dx": None, "dweight": None, "dbias": None, "dskip": None, "x": None},
                  {"x": None, "Cs": 0}, {"Cs": 0, "B": 0}, {"B": 0, "workspace": ODD}, {"workspace": ODD, "x_strides": NEG}, {"G": 3, "B": 65536}]
            if resize:
                c += [{"B": 0, "Hs": 0}, {"Hs": 0, "Ws": 11}, {"Hs": 7, "workspace": ODD}]
        elif not backward:
            c += [{k: None} for k in ("xs", "weights", "biases", "skip", "outs", "stats", "workspace", "x_strides", "skip_strides")]
            c += _sizes(resize, True, False)
            c += [{"eps": 0.0}, {"eps": -1.0}, {"x_strides[1]": NEG}, {"x_strides[0]": FAR}, {"skip_strides": NEG}, {"workspace": ODD}]
            c += [{"x_strides[2]": NEG, "xs[0]": None}]      # the strides of a sibling past D are not looked at
            c += [{k: None} for k in ("xs[1]", "weights[0]", "biases[1]", "outs[1]")]
            c += [{"xs": None, "D": 0}, {"D": 0, "B": 0}, {"B": 0, "Cs": 0}, {"Cs": 0, "C": 32766}, {"C": 32766, "eps": 0.0}, {"eps": 0.0, "x_strides[1]": NEG},
                  {"skip_strides": NEG, "workspace": ODD}, {"workspace": ODD, "xs[1]": None}]
            if resize:
                c += [{"Cs": 0, "Hs": 0}, {"C": 32766, "Hs": 0}, {"Hs": 0, "Ws": 11}, {"Ws": 11, "eps": 0.0}]
        else:
            nothing = {"dxs": None, "dweights": None, "dbiases": None}
            nog = {f"gs[{d}]": None for d in range(BASE["D"])}
            c += [{"gs": None}]
            c += _sizes(resize, True, True)
            c += [{k: None} for k in ("xs", "weights", "biases", "x_strides", "xs[1]", "weights[0]", "biases[1]")]
            c += [nog, {**nothing, "dskip": None}, {"stats": None}, {"workspace": None}, {"workspace": ODD}, {"x_strides[1]": NEG}, {"x_strides[0]": FAR}]
            c += [{**nothing, "B": 0}]
            c += [{"gs": None, "D": 0}, {"D": 0, "xs": None}, {"Cs": 0, "C": 32766}, {"C": 32766, "xs": None}, {"xs": None, **nog}, {**nog, **nothing, "dskip": None},
                  {**nothing, "dskip": None, "stats": None}, {"stats": None, "workspace": ODD}, {"workspace": ODD, "x_strides[1]": NEG}]
            if resize:
                c += [{"Cs": 0, "Hs": 0}, {"C": 32766, "Hs": 0}, {"Hs": 0, "Ws": 11}, {"Ws": 11, "xs": None}]
        cases += [(entry, f) for f in c]
    zero = [{"B": 0}, {"C": -1}, {"G": 0}, {"H": 0}, {"W": -2}, {"G": 3}, {"B": 0, "backward": 0}, {"G": 3, "backward": 0}]
    for entry in QUERIES:
        c = list(zero)
        if "resize" in entry:
            c += [{"Hs": 0}, {"Ws": 0}, {"Hs": 2}, {"Hs": 7}, {"Ws": 4}, {"Ws": 11}]
        if "siblings" in entry:
            c += [{"D": 0}, {"D": 9}, {"D": -1}]
        cases += [(entry, f) for f in c]
    return cases


CASES = _cases()      # [(entry, fault)]; label(fault) is unique within an entry


def main():
    sys.path.insert(0, ROOT)
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    rows = []
    for entry, fault in CASES:
        code, msg = call(lib, entry, fault)
        # SGR_ERR_BAD_ARG or SGR_ERR_UNSUPPORTED: an accepted call would launch on fake pointers
        assert code == 0 if entry in QUERIES else code in (-1, -2), (entry, fault, code, msg)
        assert entry in QUERIES or msg.startswith(entry.replace("_bf16", "") + ": "), (entry, fault, msg)
        rows.append(dict(entry=entry, case=label(fault), code=code, message=msg))
    assert len({(r["entry"], r["case"]) for r in rows}) == len(rows)
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print(f"{OUT}: {len(rows)} cases, {len({r['message'] for r in rows})} distinct messages from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
