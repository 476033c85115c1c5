#!/usr/bin/env python3
"""Search small inputs that reach every instantiation of stats.hip and tstats.hip.

`stat_launch_record --reach` names, per entry point its sweep starts, the
smallest input that started it: one bank, one IF, one to three blocks.  This
tool keeps the block length, the axis and the op of that input and varies the
rest (blocks per row, channels, IFs, spectra, banks, and the window in its
array: whole, a start 3 floats in, a channel step of 2, reversed channels, a
time step of 2), feeds the variants to `stat_launch_record --cases` and keeps,
of those that still start the entry point, the one with the lowest score():
first those with at least two (bank, IF) rows, then those whose launch has more
than one workgroup, then those with at least BLOCKS blocks (one per planted
class of tests/stat_planted.py), then the window form the entry point's name
hashes to, then the smallest.  Every array holds at most MAX_ELEMS elements.

Three kinds of rows follow the reach rows:
  ranks  for every quantiles entry point, the same input with 8 spread lower
         ranks (16 ranks: tests/stat_planted.py's slot classes need them); for
         k_tquantiles_split<., 3> also 4 and 7 lower ranks, whose last sweep
         holds one rank;
  tails  the channel-block selects at n = 4095, 4096, 4097, 4100 and just above
         a multiple of 256 and of 1024 (257, 260, 1025, 1028), and the
         time-block ones at 257, 1025, 4095 and 4097: the last item of a lane
         is partial.

    tools/stat_cases_gen.py path/to/stat_launch_record            > table.txt
    tools/stat_cases_gen.py path/to/stat_launch_record --write tests/stat_cases.py

--write replaces the lines between the two "# ---- generated" markers.
"""
import itertools
import re
import subprocess
import sys
import zlib

MAX_ELEMS = 1 << 20
BLOCKS = 64
KINDS = ("whole", "off3", "step2", "rev", "tstep")
NBLK0 = (2, 3, 5, 9, 17, 33, 65, 129, 257, 300)  # blocks of channels per row
NC2 = (1, 2, 3, 4, 5, 7, 8, 12, 17, 20, 33, 36, 40, 68, 132, 260, 300)  # channels, blocks of spectra


def parse_line(text):
    """(nchan, nif, ntime, window or None, axis, n, nbank, words, op)"""
    t = text.split()
    win = None if t[3] == "-" else tuple(int(x) for x in t[3].split(","))
    return (int(t[0]), int(t[1]), int(t[2]), win, int(t[4]), int(t[5]), int(t[6]), int(t[7]), t[8])


def case_line(c):
    nchan, nif, ntime, win, axis, n, nbank, words, op = c
    w = "-" if win is None else ",".join(map(str, win))
    return "%d %d %d %s %d %d %d %d %s" % (nchan, nif, ntime, w, axis, n, nbank, words, op)


def window_of(c):
    nchan, nif, ntime, win = c[:4]
    return win if win is not None else (0, nchan, 1, 0, nif, 1, 0, ntime, 1)


def place(kind, nc, ni, nt):
    """(nchan, nif, ntime, window) of an (nc, ni, nt) window of `kind`."""
    if kind == "whole":
        return nc, ni, nt, None
    if kind == "off3":
        return nc + 5, ni, nt, (3, nc, 1, 0, ni, 1, 0, nt, 1)
    if kind == "step2":
        return 2 * nc + 1, ni, nt, (1, nc, 2, 0, ni, 1, 0, nt, 1)
    if kind == "rev":
        return nc + 1, ni + 1, nt, (nc, nc, -1, 1, ni, 1, 0, nt, 1)
    return nc + 4, ni, 2 * nt, (4, nc, 1, 0, ni, 1, 1, nt, 2)


def kind_of(c):
    win = c[3]
    if win is None:
        return "whole"
    if win[2] == 2:
        return "step2"
    if win[2] == -1:
        return "rev"
    return "tstep" if win[8] == 2 else "off3"


def blocks_of(c):
    w = window_of(c)
    axis, n, nbank = c[4], max(c[5], 1), c[6]
    return (w[1] // n if axis == 0 else w[1]) * w[4] * (w[7] if axis == 0 else w[7] // n) * nbank


def variants(base):
    nchan, nif, ntime, win, axis, n, nbank, words, op = base
    yield base
    n1 = max(n, 1)
    for kind, ni, nbk in itertools.product(KINDS, (1, 2), (1, 2)):
        if axis == 0:
            for nco, nt in itertools.product(NBLK0, (1, 2, 3)):
                a = place(kind, n1 * nco, ni, nt)
                if a[0] * a[1] * a[2] <= MAX_ELEMS:
                    yield a + (axis, n, nbk, 1, op)
        else:
            for nc, nb in itertools.product(NC2, (1, 2, 3)):
                a = place(kind, nc, ni, n * nb)
                if a[0] * a[1] * a[2] <= MAX_ELEMS:
                    yield a + (axis, n, nbk, 1, op)


def score(c, sym, res):
    """Lower is better."""
    w = window_of(c)
    total = c[0] * c[1] * c[2] * c[6]
    rows = w[4] * c[6]
    gx = [int(d["gx"]) for d in res[2] if d["sym"] == sym][0]
    pref = zlib.crc32(sym.encode()) % len(KINDS)
    return (rows < 2, gx < 2, blocks_of(c) < BLOCKS, (KINDS.index(kind_of(c)) - pref) % len(KINDS),
            total)


def run(tool, cases):
    """[(plan words, symbols started in order, launches) or None] of the cases."""
    r = subprocess.run([tool, "--cases"], input="\n".join(case_line(c) for c in cases) + "\n",
                       capture_output=True, text=True)
    out = r.stdout.splitlines()[:-1]
    assert len(out) == len(cases), (len(out), len(cases), r.stderr[-500:])
    res = []
    for l in out:
        parts = l.split(" | ")
        if not parts[1].startswith("rc=0"):
            res.append(None)
            continue
        plan = tuple(int(x) for x in parts[1].split("plan=")[1].split(","))
        launches = [dict(kv.split("=", 1) for kv in p.split()[1:]) for p in parts[2:]]
        res.append((plan, [d["sym"] for d in launches], launches))
    return res


def best_of(tool, sym, base):
    cands = list(variants(base))
    best = None
    for c, res in zip(cands, run(tool, cands)):
        if res is None or sym not in res[1]:
            continue
        if best is None or score(c, sym, res) < score(best[0], sym, best[1]):
            best = (c, res)
    assert best is not None, sym
    return best


def spread(n, L):
    """The op of L lower ranks spread over a block of n (stat_launch_record's with_ops)."""
    return "quantiles:" + ",".join(repr((k * (n - 1) // L + 0.5) / (n - 1)) for k in range(L))


def with_block(c, n):
    """The case with blocks of n in place of its own (same count of blocks)."""
    nchan, nif, ntime, win, axis, n0, nbank, words, op = c
    w = window_of(c)
    kind = kind_of(c)
    if axis == 0:
        a = place(kind, w[1] // n0 * n, w[4], w[7])
    else:
        a = place(kind, w[1], w[4], w[7] // n0 * n)
    return a + (axis, n, nbank, words, op)


def main():
    tool = sys.argv[1]
    reach = {}
    r = subprocess.run([tool, "--reach"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]
    for l in r.stdout.splitlines():
        m = re.fullmatch(r"reach sym=(\S+) elems=(\d+) case=(.*)", l)
        if m:
            reach[m.group(1)] = (int(m.group(2)), parse_line(m.group(3)))
    rows, too_big, seen = [], {}, set()

    def add(sym, c, res, note):
        if c in seen:
            return
        seen.add(c)
        rows.append((sym,) + c[:7] + (c[8], res[0], res[1][0], note))

    chosen = {}
    for sym in sorted(reach):
        elems, base = reach[sym]
        if elems > MAX_ELEMS:
            too_big[sym] = "the smallest swept input that starts it holds %d elements (%s)" % (
                elems, case_line(base).strip())
            continue
        if base[8] == "var" and zlib.crc32(sym.encode()) % 2:  # (the op is a run-time argument)
            base = base[:8] + ("std",)
        c, res = best_of(tool, sym, base)
        chosen[sym] = c
        add(sym, c, res, "reach")
    # ranks: the quantiles entry points with 16 ranks, and 4 and 7 lower ranks where the sweeps differ
    for sym, c in sorted(chosen.items()):
        if not c[8].startswith("quantiles:"):
            continue
        n = c[5]
        for L in (8, 7, 4) if sym.startswith("k_tquantiles_split") and sym.endswith(",3>") else (8,):
            if n - 1 < L:
                continue
            v = c[:8] + (spread(n, L),)
            res = run(tool, [v])[0]
            if res is not None and sym in res[1]:
                add(sym, v, res, "ranks")
    # tails
    ops = ("median", "mad", "quantile:0.3", None, "outliers:1")
    for axis, ns in ((0, (4095, 4096, 4097, 4100, 257, 260, 1025, 1028)), (2, (257, 1025, 4095, 4097))):
        donors = [c for s, c in sorted(chosen.items()) if c[4] == axis and c[5] > 64]
        for k, (n, op) in enumerate(itertools.product(ns, ops)):
            d = donors[k % len(donors)]
            v = with_block(d, n)
            v = v[:8] + (op or spread(n, 8),)
            if v[0] * v[1] * v[2] > MAX_ELEMS:
                v = with_block((n * 2 if axis == 0 else 20, 2, 1 if axis == 0 else n * 2, None, axis,
                                n, 2, 1, v[8]), n)
            res = run(tool, [v])[0]
            assert res is not None, v
            add(res[1][0], v, res, "tail")
    lines = ["_TABLE = ["]
    for row in rows:
        lines.append("    %r," % (row,))
    lines.append("]")
    lines.append("TOO_BIG = {")
    for sym in sorted(too_big):
        lines.append("    %r:\n        %r," % (sym, too_big[sym]))
    lines.append("}")
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 3 and sys.argv[2] == "--write":
        with open(sys.argv[3]) as f:
            src = f.read()
        head, rest = src.split("# ---- generated", 1)
        _, tail = rest.split("# ---- generated", 1)
        with open(sys.argv[3], "w") as f:
            f.write(head + "# ---- generated by tools/stat_cases_gen.py: do not edit\n" + text +
                    "# ---- generated" + tail)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
