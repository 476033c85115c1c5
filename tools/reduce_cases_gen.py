#!/usr/bin/env python3
"""Search small inputs that reach every Float32 reduce instantiation.

Feeds candidate cases (shape, window, F, T, banks, plan options) to
`reduce_launch_record --cases`, and for every instantiation the sweep
(`--reach 1 1`) starts picks one candidate that starts it too: of those with
min(F T, 1024) blocks the one with the oddest shape (score), then the smallest.
Prints the rows of tests/reduce_cases.py's table and what no candidate of at
most 2^24 elements per bank reached.

    tools/reduce_cases_gen.py path/to/reduce_launch_record [resume.pickle] > cases.txt
"""
import itertools
import os
import pickle
import re
import subprocess
import sys
import zlib

F_ALL = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 256, 320,
         384, 512, 640, 768, 1024, 2048, 4096, 8192, 65536]
T_ALL = [1, 2, 3, 4, 8, 16, 32, 48, 128, 256, 2048]
NCO = [1, 2, 3, 4, 5, 8, 16, 17, 32, 42, 64, 65, 130, 300]
NTO = [1, 2, 3, 5, 17, 33]
OPTS = {
    "row_split": (1, 2, 4), "ts_fill": (0, 1), "narrow_mis": (0, 1), "t38": (0, 1),
    "wide_split": (0, 1), "narrow_tpb": (0, 1, 2), "lane": (0, 1), "lane3": (0, 1),
    "lanet": (0, 1), "lanet_pack": (0, 1), "vec_il": (0, 1), "vec_row": (0, 1), "row_tpb": (0, 1),
    "rowt_pack": (0, 1), "rowt_small": (0, 64, 100000), "wavet": (0, 1),
    "unaligned_vec": (0, 1, 2), "row_bpack": (0, 1), "lane_bpack": (0, 1), "wave_bpack": (0, 1),
    "col3": (0, 1), "rowt_narrow8": (0, 1), "st_plain": (0, 1, 2),
}
MAX_ELEMS = 1 << 24


def strip_op(sym):
    return re.sub(r"<\d+(,|(?=>))", "<", sym, count=1)


def windows(nc, ni, nt):
    """(name, nchan, nif, ntime, window): the whole array; a start one float
    off; an odd pitch; a channel step of 2; an aligned window inside a larger
    array that starts at IF 1 and spectrum 1."""
    yield "whole", nc, ni, nt, None
    yield "off1", nc + 4, ni, nt, (1, nc, 1, 0, ni, 1, 0, nt, 1)
    yield "pitch1", nc + 1, ni, nt, (0, nc, 1, 0, ni, 1, 0, nt, 1)
    yield "step2", 2 * nc, ni, nt, (0, nc, 2, 0, ni, 1, 0, nt, 1)
    yield "inner", nc + 8, ni + 1, nt + 1, (4, nc, 1, 1, ni, 1, 1, nt, 1)


def factors(missing):
    """The (F, T) the missing instantiations can run at, where their names say."""
    fs, ts = set(), set()
    for sym in missing:
        name, args = sym[len("k_reduce_"):-1].split("<")
        a = [int(x) for x in args.split(",") if x.isdigit()]
        if name == "rowt":
            fs.add(4 * a[0]), ts.add(a[1])
        elif name in ("narrowt", "lanet", "lanes"):
            fs.add(a[0]), ts.add(a[1])
        elif name == "col3":
            fs.add(12), ts.add(a[0])
        else:
            return F_ALL, T_ALL
    return sorted(fs), sorted(ts)


def candidates(optsets, ncos, ntos, nis, nbanks, limit, above=0, fs=F_ALL, ts=T_ALL):
    for F, T, nco, ni, nb in itertools.product(fs, ts, ncos, nis, nbanks):
        # (and the time blocks that make min(F T, 1024) blocks of it, whatever the stage's limit)
        need = -(-min(F * T, 1024) // (nco * ni * nb))
        for nto in sorted(set(ntos) | {need, need + 1}):
            nc, nt = nco * F, nto * T
            for wname, nchan, nif, ntime, win in windows(nc, ni, nt):
                size = nchan * nif * ntime
                if not above < size <= (MAX_ELEMS if nto in (need, need + 1) else limit):
                    continue
                for o in optsets:
                    yield (nchan, nif, ntime, win, F, T, nb, int(nb > 1), o)


def line(c, op=0):
    nchan, nif, ntime, win, F, T, nb, st, o = c
    w = "-" if win is None else ",".join(map(str, win))
    return "%d %d %d %s %d %d %d %d %d %s" % (nchan, nif, ntime, w, F, T, op, nb, st,
                                              " ".join("%s:%d" % kv for kv in o))


def run(tool, cases, missing, best, chunk=400000):
    """best[op-less symbol of `missing`] = (case, plan, query, kernel, first
    symbol) of the lowest score() among the cases whose launches start it."""
    cases = iter(cases)
    while True:
        part = list(itertools.islice(cases, chunk))
        if not part:
            return
        r = subprocess.run([tool, "--cases"], input="\n".join(line(c) for c in part) + "\n",
                           capture_output=True, text=True)
        out = r.stdout.splitlines()[:-1]
        assert len(out) == len(part), (len(out), len(part), r.stderr[-500:])
        for c, l in zip(part, out):
            parts = l.split(" | ")
            if len(parts) < 3 or not parts[1].startswith("rc=0"):
                continue
            for lp in parts[2:]:
                sym = strip_op(lp.split("sym=")[1])
                if sym in missing and (sym not in best or score(c, sym) < score(best[sym][0], sym)):
                    f = dict(kv.split("=", 1) for kv in parts[1].split())
                    main = strip_op(parts[2].split("sym=")[1])
                    best[sym] = (c, f["plan"], f["query"], f["kernel"], main)


WINDOWS = ("whole", "off1", "pitch1", "step2", "inner")


def window_name(win):
    if win is None:
        return "whole"
    return "step2" if win[2] == 2 else "off1" if win[0] == 1 else "inner" if win[0] == 4 else "pitch1"


def score(c, sym):
    """Lower is better: enough blocks, few options, the window this symbol
    prefers (so that the table's windows vary) and an odd shape unless that costs
    a million elements, a small input."""
    nchan, nif, ntime, win, F, T, nb, st, o = c
    nc, ni, nt = (nchan, nif, ntime) if win is None else (win[1], win[4], win[7])
    nco, nto = nc // F, nt // T
    enough = nco * ni * nto * nb >= min(F * T, 1024)
    # points for what kernels get wrong: a width that is no power of two, several
    # waves' worth of groups, more than one 1024-channel column block with a
    # partial last one, several time blocks, two IFs
    odd = ((nco & (nco - 1) != 0) + (nco >= 17) + (nc > 1024 and nc % 1024 != 0) + (nto >= 3) +
           (ni == 2))
    prefers = WINDOWS[zlib.crc32(sym.encode()) % len(WINDOWS)]
    size = nchan * nif * ntime * nb
    return (not enough, len(o), size >> 20, -odd, window_name(win) != prefers, size)


def main():
    tool = sys.argv[1]
    want = set()
    for l in subprocess.run([tool, "--reach", "1", "1"], capture_output=True,
                            text=True).stdout.splitlines():
        if l.startswith("reach sym=k_reduce_"):
            want.add(strip_op(l.split()[1][4:]))
    singles = [((k, v),) for k, vs in OPTS.items() for v in vs]
    pairs = [a + b for a in (singles[k] for k, s in enumerate(singles)
                             if s[0][0] in ("rowt_small", "t38", "unaligned_vec"))
             for b in singles if b[0][0] != a[0][0]]
    triples = [(("rowt_small", 0), ("rowt_narrow8", 0)) + s for s in singles
               if s[0][0] not in ("rowt_small", "rowt_narrow8")]
    # (the last stage: k_reduce_rows and the time-chunked plans want >= 4096 waves
    # or long time blocks, whatever the options)
    splits = [()] + [s for s in singles if s[0][0] in ("row_split", "wide_split", "ts_fill")]
    stages = [
        ([()], NCO, NTO, [1, 2], [1, 2, 4, 8], 1 << 20, 0),
        (singles, [1, 3, 4, 8, 16, 17, 65, 300], [1, 3, 17], [1, 2], [1, 8], 1 << 18, 0),
        (splits, [1, 2, 3, 16, 17, 33, 66, 132, 264, 528, 1056, 2112], [1, 2, 3, 16, 17], [1],
         [1, 8], MAX_ELEMS, 1 << 18),
        (pairs + triples, [1, 2, 3, 4, 8, 16, 17, 65, 516], [1, 3, 17], [1, 2], [1, 4, 8], 1 << 16,
         0),
    ]
    best = {}
    if len(sys.argv) > 2 and os.path.exists(sys.argv[2]):  # (a search resumed)
        with open(sys.argv[2], "rb") as f:
            best = {k: v for k, v in pickle.load(f).items() if k in want}
    for optsets, ncos, ntos, nis, nbanks, limit, above in stages:
        missing = want - set(best)
        if not missing:
            break
        fs, ts = factors(missing) if len(optsets[0]) > 1 else (F_ALL, T_ALL)
        run(tool, candidates(optsets, ncos, ntos, nis, nbanks, limit, above, fs, ts), missing, best)
        print("# stage: %d of %d reached" % (len(best), len(want)), file=sys.stderr)
        if len(sys.argv) > 2:
            with open(sys.argv[2], "wb") as f:
                pickle.dump(best, f)
    chosen, seen = [], set()
    for sym in sorted(best):
        c, plan, query, kernel, main = best[sym]
        if c in seen:
            continue
        seen.add(c)
        chosen.append((kernel, main, c, plan, query))
    chosen.sort(key=lambda x: (x[0], x[2][4], x[2][5], x[1]))
    for kernel, main, c, plan, query in chosen:
        nchan, nif, ntime, win, F, T, nb, st, o = c
        print("    (%r, %d, %d, %d, %r, %d, %d, %d, %d, %r, (%s), (%s))," % (
            main[len("k_reduce_"):], nchan, nif, ntime, win, F, T, nb, st, o,
            plan.replace(",", ", "), query.replace(",", ", ")))
    for sym in sorted(want - set(best)):
        print("# not reached: %s" % sym)


if __name__ == "__main__":
    main()
