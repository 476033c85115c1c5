"""A plain statement of HDF5 filter 32008 (bitshuffle + LZ4), independent of
libbldp_hip and of oracle/, and the conformance corpus built from it
(tests/test_bslz4_conformance.py, tools/bslz4_host_check.cpp).

The LZ4 block format, as its specification states it.  A block is a list of
sequences.  A sequence is
    token          high nibble: literal count, low nibble: match length - 4
    [length bytes] when the literal nibble is 15: bytes added to the count,
                   the last one being the first that is not 255
    literals
    offset         16-bit little-endian, 1..65535, counted back from the
                   current output position
    [length bytes] when the match nibble is 15, as above
and the match copies `match length` bytes from `offset` bytes back, byte by
byte, so a match may read bytes it has itself just written (offset < length).
The last sequence stops after its literals.  A decoder stops when the input
is used up: after the literals of a sequence (the usual end) or after a match
(a block ending on a match, which the format's compressor-side end rules
forbid a compressor to write but which leaves a decoder nothing undefined to
do; the decoders here accept it, and the corpus pins that).

    python tests/bslz4_ref.py --dump FILE

writes every chunk of the corpus (directed, malformed, mutated) with its
element size, verdict and expected bytes, for the stand-alone host check.
"""
from __future__ import annotations

import struct
import sys

import numpy as np

HEADER = 12
# the largest block (elements) the GPU decoder's LDS plan admits, per element
# size: lz4_bound(block bytes) and the block bytes, each rounded up to 16,
# within 64 KiB
MAX_BLOCK = {4: 8168, 2: 16344, 1: 32688, 8: 4080}
ABOVE_PLAN = 8176  # Float32 elements: one transpose group more than the plan admits


class Malformed(ValueError):
    """What a decoder must refuse."""


# --------------------------------------------------------------------------- LZ4


def _length_bytes(extra: int) -> bytes:
    """The bytes that follow a nibble of 15: `extra` = length - 15 >= 0."""
    return b"\xff" * (extra // 255) + bytes([extra % 255])


def emit_sequence(nlit: int, lits: bytes, off, ml) -> bytes:
    """One sequence as the format writes it.  `nlit` is the declared literal
    count (the malformed cases declare another count than len(lits)); off None
    ends the sequence after its literals."""
    mcode = 0 if off is None else ml - 4
    assert mcode >= 0
    token = (min(nlit, 15) << 4) | min(mcode, 15)
    s = bytes([token])
    if nlit >= 15:
        s += _length_bytes(nlit - 15)
    s += bytes(lits)
    if off is not None:
        s += struct.pack("<H", off)
        if mcode >= 15:
            s += _length_bytes(mcode - 15)
    return s


class SeqBuilder:
    """One LZ4 block from an explicit list of sequences, with the bytes a
    decoder must produce tracked alongside."""

    def __init__(self):
        self.block = bytearray()
        self.out = bytearray()
        self.ended = False  # a literal-only sequence was written

    def seq(self, lits: bytes = b"", off=None, ml=None) -> "SeqBuilder":
        assert not self.ended, "a literal-only sequence ends the block"
        lits = bytes(lits)
        self.block += emit_sequence(len(lits), lits, off, ml)
        self.out += lits
        if off is None:
            self.ended = True
            return self
        assert ml >= 4 and 1 <= off <= min(len(self.out), 65535), (off, ml, len(self.out))
        dst = self.out
        op = len(dst)
        dst.extend(bytes(ml))
        for i in range(ml):  # byte by byte: the source may overlap the destination
            dst[op + i] = dst[op - off + i]
        return self

    def fill(self, nbytes: int, rng) -> "SeqBuilder":
        """Random literals up to `nbytes` of output; nothing when the block is
        already full (it then ends on its last match)."""
        left = nbytes - len(self.out)
        assert left >= 0, (nbytes, len(self.out))
        if left:
            self.seq(rand_bytes(rng, left))
        return self


def rand_bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def ref_lz4_decode(block: bytes, nbytes: int) -> bytes:
    """Decode one LZ4 block that must give exactly `nbytes`; Malformed
    otherwise."""
    src = bytes(block)
    n = len(src)
    out = bytearray()
    ip = 0

    def length(base: int, ip: int):
        if base == 15:
            while True:
                if ip >= n:
                    raise Malformed("length bytes cut off")
                b = src[ip]
                ip += 1
                base += b
                if b != 255:
                    break
        return base, ip

    while ip < n:
        token = src[ip]
        ip += 1
        lit, ip = length(token >> 4, ip)
        if ip + lit > n:
            raise Malformed("literals past the input")
        if len(out) + lit > nbytes:
            raise Malformed("literals past the output")
        for i in range(lit):
            out.append(src[ip + i])
        ip += lit
        if ip == n:
            break  # the last sequence: literals only
        if ip + 2 > n:
            raise Malformed("offset cut off")
        off = src[ip] | src[ip + 1] << 8
        ip += 2
        ml, ip = length(token & 15, ip)
        ml += 4
        if off == 0:
            raise Malformed("offset 0")
        if off > len(out):
            raise Malformed("offset before the block's first byte")
        if len(out) + ml > nbytes:
            raise Malformed("match past the output")
        for i in range(ml):
            out.append(out[len(out) - off])
    if len(out) != nbytes:
        raise Malformed(f"block gives {len(out)} bytes, not {nbytes}")
    return bytes(out)


def lz4_literals(data: bytes) -> bytes:
    """The block that stores `data` as one run of literals."""
    return bytes(SeqBuilder().seq(data).block)


def lz4_greedy(data: bytes) -> bytes:
    """A small greedy compressor on SeqBuilder: the latest earlier position of
    each 4-byte group, matches extended as far as they go (overlapping ones
    included).  It keeps none of the format's end-of-block rules, which bind
    compressors and not decoders."""
    data = bytes(data)
    n = len(data)
    sb = SeqBuilder()
    last = {}
    i = lit0 = 0
    while i + 4 <= n:
        key = data[i:i + 4]
        j = last.get(key)
        last[key] = i
        if j is None or i - j > 65535:
            i += 1
            continue
        ml = 4
        while i + ml < n and data[j + ml] == data[i + ml]:
            ml += 1
        sb.seq(data[lit0:i], i - j, ml)
        i += ml
        lit0 = i
    if lit0 < n:
        sb.seq(data[lit0:])
    assert bytes(sb.out) == data
    return bytes(sb.block)


# --------------------------------------------------------------------- bitshuffle


def shuffle(a: np.ndarray, es=None) -> bytes:
    """Bit planes of n elements (n % 8 == 0): plane r = bit r % 8 of byte r // 8
    of every element, packed LSB-first, plane r at byte r * n / 8."""
    es = a.dtype.itemsize if es is None else es
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1, es)
    assert b.shape[0] % 8 == 0
    bits = np.unpackbits(b[:, :, None], axis=2, bitorder="little")  # (n, es, 8)
    return np.packbits(bits.transpose(1, 2, 0), axis=2, bitorder="little").tobytes()


def unshuffle(planes: bytes, n: int, es: int) -> bytes:
    """The n elements of es bytes whose bit planes `planes` holds."""
    assert n % 8 == 0 and len(planes) == n * es, (n, es, len(planes))
    p = np.frombuffer(bytes(planes), np.uint8).reshape(es, 8, n // 8)
    bits = np.unpackbits(p, axis=2, bitorder="little")  # (es, 8, n)
    return np.packbits(bits.transpose(2, 0, 1), axis=2, bitorder="little").tobytes()


# ------------------------------------------------------------------------- chunks


def block_sizes(n: int, block_elems: int):
    """Elements of every LZ4 block of an n-element chunk, and of its raw tail."""
    sizes = [block_elems] * (n // block_elems)
    last = n % block_elems
    last -= last % 8
    if last:
        sizes.append(last)
    return sizes, n - sum(sizes)


def make_chunk(blocks, tail_bytes: bytes, n: int, block_elems: int, es: int) -> bytes:
    """Header (uint64 BE bytes, uint32 BE block bytes), a uint32 BE size and the
    LZ4 bytes per block, the raw tail."""
    c = struct.pack(">QI", n * es, block_elems * es)
    for b in blocks:
        c += struct.pack(">I", len(b)) + bytes(b)
    return c + bytes(tail_bytes)


def encode(a: np.ndarray, block_elems: int, lz4=lz4_greedy, es=None) -> bytes:
    """The chunk of `a` (any dtype; es overrides the element size for byte
    arrays that hold wider elements)."""
    es = a.dtype.itemsize if es is None else es
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1, es)
    n = b.shape[0]
    sizes, tail = block_sizes(n, block_elems)
    blocks, e = [], 0
    for ne in sizes:
        blocks.append(lz4(shuffle(b[e:e + ne], es)))
        e += ne
    return make_chunk(blocks, b[e:].tobytes(), n, block_elems, es)


def ref_decode_chunk(chunk: bytes, es: int) -> bytes:
    """The bytes of a chunk, or Malformed."""
    chunk = bytes(chunk)
    if len(chunk) < HEADER:
        raise Malformed("chunk shorter than its header")
    nb, bb = struct.unpack(">QI", chunk[:HEADER])
    if nb % es or bb % es or bb == 0 or (bb // es) % 8:
        raise Malformed("bad header")
    n = nb // es
    sizes, tail = block_sizes(n, bb // es)
    pos, out = HEADER, b""
    for ne in sizes:
        if pos + 4 > len(chunk):
            raise Malformed("block size cut off")
        cl, = struct.unpack(">I", chunk[pos:pos + 4])
        if pos + 4 + cl > len(chunk):
            raise Malformed("block overruns the chunk")
        out += unshuffle(ref_lz4_decode(chunk[pos + 4:pos + 4 + cl], ne * es), ne, es)
        pos += 4 + cl
    if pos + tail * es != len(chunk):
        raise Malformed("tail of the wrong size")
    return out + chunk[pos:]


# ------------------------------------------------------------------------- corpus


class Case:
    """One chunk of the corpus: `want` is the bytes a decoder must give, or None
    when it must refuse the chunk."""

    def __init__(self, name, es, chunk, want, block_elems):
        self.name, self.es, self.chunk, self.want = name, es, bytes(chunk), want
        self.block_elems = block_elems

    def __repr__(self):
        return f"Case({self.name}, es={self.es})"


def chunk_of(name, es, block_elems, builders, tail_elems=0, rng=None) -> Case:
    """A chunk of full blocks from SeqBuilders (each holding block_elems * es
    plane bytes), checked against ref_lz4_decode before anything else sees it."""
    want = b""
    for sb in builders:
        assert len(sb.out) == block_elems * es, (name, len(sb.out), block_elems * es)
        assert ref_lz4_decode(sb.block, len(sb.out)) == bytes(sb.out), name
        want += unshuffle(sb.out, block_elems, es)
    tail = rand_bytes(rng, tail_elems * es) if tail_elems else b""
    n = block_elems * len(builders) + tail_elems
    return Case(name, es, make_chunk([sb.block for sb in builders], tail, n, block_elems, es),
                want + tail, block_elems)


GRID_OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256)
LITERAL_RUNS = (0, 1, 14, 15, 16, 269, 270, 271, 525)


def grid_lengths(o: int, nbytes: int):
    cand = (4, 5, o - 1, o, o + 1, 2 * o, 2 * o + 1, 63, 64, 65, 127, 128, 129, 18, 19, 273, 274,
            529)
    return sorted({m for m in cand if m >= 4 and o + m <= nbytes})


def grid_cases(es: int, rng):
    """Offset x length: o literals, one match (o, ml), literals to the end; one
    chunk per offset, one block per length."""
    be = 512
    out = []
    for o in GRID_OFFSETS:
        sbs = [SeqBuilder().seq(rand_bytes(rng, o), o, ml).fill(be * es, rng)
               for ml in grid_lengths(o, be * es)]
        out.append(chunk_of(f"grid_o{o}_es{es}", es, be, sbs))
    return out


def literal_cases(es: int, rng):
    """Literal runs on the 15 and 15 + 255 k boundaries, in the middle of a
    block (a run of 0 after a first sequence) and as its last sequence (a run
    of 0 there is a block ending on a match)."""
    be = 1024
    nb = be * es
    mid, end = [], []
    for r in LITERAL_RUNS:
        mid.append(SeqBuilder().seq(rand_bytes(rng, 8), 5, 9).seq(rand_bytes(rng, r), 3, 7)
                   .fill(nb, rng))
        sb = SeqBuilder().seq(rand_bytes(rng, 24), 24, nb - 24 - r)
        if r:
            sb.seq(rand_bytes(rng, r))
        end.append(sb)
    return [chunk_of(f"literals_mid_es{es}", es, be, mid),
            chunk_of(f"literals_end_es{es}", es, be, end)]


def chain_cases(es: int, rng):
    be = 512
    nb = be * es
    inside = (SeqBuilder().seq(rand_bytes(rng, 32), 32, 40)  # writes [32, 72)
              .seq(b"", 20, 16).fill(nb, rng))               # reads [52, 68)
    straddle = (SeqBuilder().seq(rand_bytes(rng, 32), 32, 20)  # match writes [32, 52)
                .seq(rand_bytes(rng, 10), 20, 16).fill(nb, rng))  # reads [42, 58) over [52, 62)
    four = SeqBuilder().seq(rand_bytes(rng, 70), 5, 4)
    for off, ml in ((1, 10), (64, 100), (3, 7), (65, 131)):
        four.seq(b"", off, ml)
    four.fill(nb, rng)
    ends = SeqBuilder().seq(rand_bytes(rng, 40), 17, nb - 40)  # the block ends on a match
    assert not ends.ended
    return [chunk_of(f"chain_es{es}", es, be, [inside, straddle, four]),
            chunk_of(f"ends_on_match_es{es}", es, be, [ends])]


def small_block_cases(es: int, rng):
    """Blocks of one transpose group (8 elements) and of 64 elements."""
    out = []
    for be in (8, 64):
        nb = be * es
        sbs = [SeqBuilder().fill(nb, rng),
               SeqBuilder().seq(rand_bytes(rng, 4), 4, nb - 4),
               SeqBuilder().seq(rand_bytes(rng, 1), 1, 4).fill(nb, rng),
               SeqBuilder().seq(rand_bytes(rng, 3), 2, 5).fill(nb, rng)]
        out.append(chunk_of(f"block{be}_es{es}", es, be, sbs, tail_elems=5, rng=rng))
    return out


def largest_block(nbytes: int, rng) -> SeqBuilder:
    """A block of the largest size with matches from its first byte
    (offset = op), from 16385 and from 32000 bytes back."""
    sb = SeqBuilder().seq(rand_bytes(rng, 100), 100, 50)
    sb.seq(rand_bytes(rng, 16385 - 150), 16385, 300)     # op 16385: reads [0, 300)
    sb.seq(rand_bytes(rng, 17000 - len(sb.out)), 16385, 64)
    sb.seq(rand_bytes(rng, 32000 - len(sb.out)), 32000, 200)  # op 32000: reads [0, 200)
    sb.seq(rand_bytes(rng, 37), 32000, 19)
    return sb.fill(nbytes, rng)


def largest_cases(es: int, rng):
    be = MAX_BLOCK[es]
    return [chunk_of(f"largest_es{es}", es, be, [largest_block(be * es, rng)], tail_elems=3,
                     rng=rng)]


def above_plan_case(rng) -> Case:
    return chunk_of("above_plan_es4", 4, ABOVE_PLAN, [largest_block(ABOVE_PLAN * 4, rng)])


def geometry_cases(es: int, rng):
    """n around the block and the transpose group; n = 0 is a bare header and
    n < 8 a raw tail alone."""
    be = 64
    out = []
    for n in (0, 1, 7, 8, 9, be - 1, be, be + 7, be + 8, 2 * be + 15):
        a = rng.integers(0, 3, (n, es)).astype(np.uint8)  # few values: real matches
        c = encode(a, be, lz4_greedy, es)
        assert ref_decode_chunk(c, es) == a.tobytes()
        out.append(Case(f"n{n}_es{es}", es, c, a.tobytes(), be))
    return out


def es3_case(rng) -> Case:
    a = rng.integers(0, 4, (74, 3)).astype(np.uint8)
    c = encode(a, 32, lz4_greedy, 3)
    assert ref_decode_chunk(c, 3) == a.tobytes()
    return Case("n74_es3", 3, c, a.tobytes(), 32)


def directed_cases():
    """Every valid directed chunk, by element size (the es = 3 chunk and the
    block above the LDS plan are apart: es3_case, above_plan_case)."""
    rng = np.random.default_rng(20240)
    out = []
    for es in (4, 1, 2, 8):
        for f in (grid_cases, literal_cases, chain_cases, small_block_cases, largest_cases,
                  geometry_cases):
            out += f(es, rng)
    return out


def _raw_chunk(block: bytes, n=64, be=64, es=4, tail=b"", size=None, nb=None, bb=None) -> bytes:
    c = struct.pack(">QI", n * es if nb is None else nb, be * es if bb is None else bb)
    return c + struct.pack(">I", len(block) if size is None else size) + block + tail


def malformed_cases():
    """One chunk per check a decoder must make (Float32, one block of 64
    elements = 256 plane bytes unless the header is the subject).  Apart from
    the one fault each block is well formed and of the right length, so it
    can be refused for that fault alone.  `where` says which layer refuses it
    on the device: "block" (k_bslz4), "plan" (k_bslz4_plan) or "header" (the
    host, before any launch)."""
    rng = np.random.default_rng(20241)
    nb = 256
    r = lambda k: rand_bytes(rng, k)  # noqa: E731
    seq = emit_sequence
    good = SeqBuilder().seq(r(8), 8, 8).fill(nb, rng)
    blocks = {
        # lits 8, a match of 8 that would be fine at offset 8, 240 literals
        "offset_0": seq(8, r(8), 0, 8) + seq(240, r(240), None, None),
        "offset_op_plus_1": seq(8, r(8), 9, 8) + seq(240, r(240), None, None),
        "offset_at_op_0": seq(0, b"", 1, 8) + seq(248, r(248), None, None),
        # a run that declares 20 literals where 10 bytes are left
        "literals_past_input": seq(8, r(8), 8, 8) + seq(20, r(10), None, None),
        # 60 literals, all present, where 48 bytes of output are left
        "literals_past_output": seq(8, r(8), 8, 200) + seq(60, r(60), None, None),
        "match_past_output": seq(8, r(8), 8, 300),
        # the literal count's / match length's 255 is the block's last byte
        "literal_length_cut": seq(8, r(8), 8, 8) + b"\xf0\xff",
        "match_length_cut": seq(8, r(8), 8, 19 + 255)[:-1],
        "offset_cut": seq(8, r(8), 8, 8)[:-1],
        "one_byte_short": seq(8, r(8), 8, 8) + seq(239, r(239), None, None),
        "one_byte_long": seq(8, r(8), 8, 8) + seq(241, r(241), None, None),
        "one_byte_long_match": seq(8, r(8), 8, 249),
    }
    assert blocks["match_length_cut"][-1] == 0xFF and blocks["literal_length_cut"][-1] == 0xFF
    out = [Case(k, 4, _raw_chunk(b), None, 64) for k, b in blocks.items()]
    for c in out:
        c.where = "block"
    plan = {
        # 300 literals, all present, in a 256-byte block: past the output, and
        # a block longer than any LZ4 block of 256 bytes can be (the GPU
        # planner's staging bound, lz4_bound)
        "block_longer_than_bound": _raw_chunk(seq(8, r(8), 8, 8)
                                              + seq(300, r(300), None, None)),
        "block_size_overruns": _raw_chunk(bytes(good.block), size=len(good.block) + 1),
        "trailing_bytes": _raw_chunk(bytes(good.block), n=67, tail=r(12) + b"\0"),
        "tail_one_short": _raw_chunk(bytes(good.block), n=67, tail=r(8)),
    }
    header = {
        "bytes_not_multiple_of_es": _raw_chunk(bytes(good.block), nb=257),
        "block_not_multiple_of_8": _raw_chunk(bytes(good.block), bb=4 * 60),
        "block_bytes_0": _raw_chunk(bytes(good.block), bb=0),
    }
    for where, d in (("plan", plan), ("header", header)):
        for k, c in d.items():
            case = Case(k, 4, c, None, 64)
            case.where = where
            out.append(case)
    # the faultless chunk the others are variations of
    ok = Case("malformed_base_ok", 4, _raw_chunk(bytes(good.block)), unshuffle(good.out, 64, 4), 64)
    ok.where = None
    for c in out:
        try:
            ref_decode_chunk(c.chunk, c.es)
        except Malformed:
            continue
        raise AssertionError(f"{c.name}: the reference accepts it")
    assert ref_decode_chunk(ok.chunk, 4) == ok.want
    return out, ok


MUTATION_SEED = 7
MUTATIONS_PER_CHUNK = 50


def mutation_bases():
    """Four small valid chunks (blocks of 64 elements, several blocks and a
    tail).  Two are mostly literals with a few short and overlapping matches
    (element sizes 4 and 2: most changed bytes are literals, and decode to
    other bytes); two are chains of short sequences, little but tokens,
    offsets and lengths (element sizes 1 and 8: most changed tokens and
    lengths break the block)."""
    rng = np.random.default_rng(20242)
    out = []
    for es in (4, 2):
        nb = 64 * es
        sbs = [SeqBuilder().seq(rand_bytes(rng, 12), 12, 20).seq(rand_bytes(rng, 5), 1, 9)
               .fill(nb, rng),
               SeqBuilder().seq(rand_bytes(rng, 16), 3, 19).seq(b"", 30, 6).fill(nb, rng)]
        out.append(chunk_of(f"mutation_base_es{es}", es, 64, sbs, tail_elems=3, rng=rng))
    for es, nblock in ((1, 3), (8, 1)):
        nb = 64 * es
        sbs = []
        for _ in range(nblock):
            sb = SeqBuilder().seq(rand_bytes(rng, 2), 1, 4)
            while nb - len(sb.out) >= 14:
                sb.seq(rand_bytes(rng, int(rng.integers(0, 2))),
                       int(rng.integers(1, len(sb.out) + 1)), int(rng.integers(4, 13)))
            sbs.append(sb.fill(nb, rng))
        out.append(chunk_of(f"mutation_base_es{es}", es, 64, sbs, tail_elems=1, rng=rng))
    return out


def mutation_cases(seed: int = MUTATION_SEED):
    """MUTATIONS_PER_CHUNK single-byte changes of each base chunk, after the
    12-byte header (the header has directed cases of its own, and the device
    refuses block sizes the host accepts).  The verdict and the bytes are the
    reference decoder's."""
    rng = np.random.default_rng(seed)
    out = []
    for base in mutation_bases():
        for k in range(MUTATIONS_PER_CHUNK):
            pos = int(rng.integers(HEADER, len(base.chunk)))
            c = bytearray(base.chunk)
            c[pos] ^= int(rng.integers(1, 256))
            try:
                want = ref_decode_chunk(c, base.es)
            except Malformed:
                want = None
            out.append(Case(f"{base.name}_m{k}_at{pos}", base.es, c, want, 64))
    return out


def dump(path: str) -> int:
    """Corpus file for tools/bslz4_host_check.cpp, little-endian:
    "BSLZ4COR", uint32 count, then per chunk uint32 es, uint32 verdict
    (1 = decodes), uint64 chunk bytes, uint64 expected bytes, the chunk, the
    expected bytes."""
    rng = np.random.default_rng(20243)
    bad, ok = malformed_cases()
    cases = directed_cases() + [es3_case(rng), above_plan_case(rng), ok] + bad + mutation_cases()
    with open(path, "wb") as f:
        f.write(b"BSLZ4COR" + struct.pack("<I", len(cases)))
        for c in cases:
            want = c.want if c.want is not None else b""
            f.write(struct.pack("<IIQQ", c.es, int(c.want is not None), len(c.chunk), len(want)))
            f.write(c.chunk)
            f.write(want)
    return len(cases)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit(__doc__)
    print(f"{dump(sys.argv[2])} chunks -> {sys.argv[2]}")
