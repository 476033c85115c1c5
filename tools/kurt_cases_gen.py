#!/usr/bin/env python3
"""Search small inputs that reach every instantiation of kurtosis.hip.

`kurt_launch_record --reach` names, per entry point its sweep starts, the
smallest input that started it.  That input is one bank of four channels (or
one) and one IF.  This tool first lengthens it to the largest odd count of
spectra, of the next 63, that still starts the entry point (fill_registers),
then varies it (channels, IFs, banks, blocks, the window in its array, a dense
or a strided result), keeping the order and the plan options, feeds the variants to
`kurt_launch_record --cases` and keeps, of those that still start the entry
point, the one with the lowest score(): first those with at least two (bank,
IF) rows that hold all four row kinds of tests/kurt_planted.py (whatever
their size, within 2^25 elements per bank: up to four banks are tried); then
inputs of up to 2^22 elements over all banks count as equally small, and
among them the one wins that has two banks, two IFs, many (bank, IF, channel) rows for tests/kurt_planted.py's planted
rows, several channel tiles with a partial last one, and three or more blocks.
Entry points whose smallest swept input exceeds 2^25 elements per bank go to
TOO_BIG.

    tools/kurt_cases_gen.py path/to/kurt_launch_record            > table.txt
    tools/kurt_cases_gen.py path/to/kurt_launch_record --write tests/kurt_cases.py

--write replaces the lines between the two "# ---- generated" markers.
"""
import itertools
import re
import subprocess
import sys
import zlib

MAX_ELEMS = 1 << 25  # per bank
SMALL = 22  # inputs of up to 2^SMALL elements over all banks: equally small
NC_VEC = (4, 8, 12, 20, 36, 68, 132, 260)
NC_ODD = (1, 3, 5, 7, 9, 13, 33, 65, 67, 129, 131, 257)
KINDS = ("whole", "off1", "pitch1", "step2", "inner")


def parse_line(text):
    """(nchan, nif, ntime, window or None, order, tblock, nbank, dense, options)"""
    t = text.split()
    win = None if t[3] == "-" else tuple(int(x) for x in t[3].split(","))
    opts = tuple((o.split(":")[0], int(o.split(":")[1])) for o in t[8:])
    return (int(t[0]), int(t[1]), int(t[2]), win, int(t[4]), int(t[5]), int(t[6]), int(t[7]), opts)


def case_line(c):
    nchan, nif, ntime, win, order, tblock, nbank, dense, opts = c
    w = "-" if win is None else ",".join(map(str, win))
    return "%d %d %d %s %d %d %d %d %s" % (nchan, nif, ntime, w, order, tblock, nbank, dense,
                                           " ".join("%s:%d" % kv for kv in opts))


def window_of(c):
    nchan, nif, ntime, win = c[:4]
    return win if win is not None else (0, nchan, 1, 0, nif, 1, 0, ntime, 1)


def kind_of(c):
    win = c[3]
    if win is None:
        return "whole"
    if win[2] == 2:
        return "step2"
    if win[0] == 4:
        return "inner"
    return "off1" if win[0] == 1 else "pitch1"


def place(kind, nc, ni, nt):
    """(nchan, nif, ntime, window): the window of `kind` in its array: whole; a
    start one float off; an odd pitch; a channel step of 2; inside a larger
    array, from IF 1 and spectrum 1."""
    if kind == "whole":
        return nc, ni, nt, None
    if kind == "off1":
        return nc + 4, ni, nt, (1, nc, 1, 0, ni, 1, 0, nt, 1)
    if kind == "pitch1":
        return nc + 1, ni, nt, (0, nc, 1, 0, ni, 1, 0, nt, 1)
    if kind == "step2":
        return 2 * nc, ni, nt, (0, nc, 2, 0, ni, 1, 0, nt, 1)
    return nc + 8, ni + 1, nt + 1, (4, nc, 1, 1, ni, 1, 1, nt, 1)


def with_spectra(base, spectra):
    """`base` with `spectra` per window (tblock = 0) or per block, its block count kept."""
    nchan, nif, ntime, win, order, tblock, nbank, dense, opts = base
    w = window_of(base)
    nb = w[7] // tblock if tblock else 1
    grow = spectra * nb - w[7]
    if win is not None:
        win = win[:7] + (spectra * nb,) + win[8:]
    return (nchan, nif, ntime + grow, win, order, spectra if tblock else 0, nbank, dense, opts)


def fill_registers(tool, sym, base):
    """The reach's input is the fewest spectra that start `sym` (a single
    spectrum for the smallest forms, whose every result is NaN): take instead the
    largest odd count of the next 63 that still starts it, so that a register
    form runs nearly full, with waves and batches of unequal counts."""
    w = window_of(base)
    s0 = base[5] if base[5] else w[7]
    if w[7] == 0:
        return base
    cands = [with_spectra(base, s0 + d) for d in range(64)]
    ok = [c for c, res in zip(cands, run(tool, cands)) if res is not None and sym in res[1]]
    odd = [c for c in ok if (c[5] if c[5] else window_of(c)[7]) % 2 == 1]
    return (odd or ok)[-1]


def variants(base):
    nchan, nif, ntime, win, order, tblock, nbank, dense, opts = base
    w = window_of(base)
    nc, nt = w[1], w[7]
    yield base
    if nt == 0:  # (the NaN fill: the reach's own window)
        return
    spectra = tblock if tblock else nt
    nbs = sorted({nt // tblock, 2, 3, 5}) if tblock else [1]
    ncs = sorted(set((NC_VEC if nc % 4 == 0 else NC_ODD) + (nc,)))
    for kind, c, ni, nb, nbk, dn in itertools.product(KINDS, ncs, (1, 2, 3), nbs, (1, 2, 3, 4),
                                                      (1, 0)):
        if not dn and (nbk != 1 or (order == 4 and tblock == 0)):
            continue
        a = place(kind, c, ni, spectra * nb)
        if a[0] * a[1] * a[2] > MAX_ELEMS:
            continue
        yield a + (order, tblock, nbk, dn, opts)


def score(c, sym):
    """Lower is better."""
    nchan, nif, ntime, win, order, tblock, nbank, dense, opts = c
    w = window_of(c)
    nc, ni, nt = w[1], w[4], w[7]
    total = nchan * nif * ntime * nbank
    rows = nc * ni * nbank
    h = zlib.crc32(sym.encode())
    want_dense = 0 if h % 3 == 0 else 1
    groups = ni * nbank  # (bank, IF) rows
    # tests/kurt_planted.py's kind of channel c of row g is (c + (g if nc < 4 else 0)) % 4
    kinds = {(c + (g if nc < 4 else 0)) % 4 for c in range(min(nc, 4)) for g in range(groups)}
    planted = groups >= 2 and len(kinds) == 4  # first of all: two rows, every row kind
    rich = ((nbank >= 2) + (ni >= 2) + (rows >= 8) + (rows >= 16) + (rows >= 32) +
            (nc > 128 and nc % 128 != 0) + (tblock > 0 and nt // tblock >= 3))
    return (not planted, total >> SMALL if total > 1 << SMALL else 0, dense != want_dense, -rich,
            kind_of(c) != KINDS[(h >> 8) % len(KINDS)], total)


def run(tool, cases):
    """[(plan words, symbols started, in order) or None] of the cases."""
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
        res.append((plan, [p.split()[1][4:] for p in parts[2:]]))
    return res


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
    for sym in sorted(reach):
        elems, base = reach[sym]
        if elems > MAX_ELEMS:
            too_big[sym] = "the smallest swept input that starts it holds %d elements per bank (%s)" % (
                elems, case_line(base).strip())
            continue
        cands = list(variants(fill_registers(tool, sym, base)))
        best = None
        for c, res in zip(cands, run(tool, cands)):
            if res is None or sym not in res[1]:
                continue
            if best is None or score(c, sym) < score(best[0], sym):
                best = (c, res)
        assert best is not None, sym
        if best[0] in seen:
            continue
        seen.add(best[0])
        rows.append((sym, best[0], best[1][0], best[1][1][0]))
    lines = ["_TABLE = ["]
    for sym, c, plan, first in rows:
        lines.append("    (%r, %d, %d, %d, %r, %d, %d, %d, %d, %r, %r, %r)," % ((sym,) + c + (plan, first)))
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
            f.write(head + "# ---- generated by tools/kurt_cases_gen.py: do not edit\n" + text +
                    "# ---- generated" + tail)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
