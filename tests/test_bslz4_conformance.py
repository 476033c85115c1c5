"""Directed conformance of the bitshuffle/LZ4 decoders (csrc/bslz4.hip) through
the C ABI alone: bldp_bslz4_info, bldp_bslz4_decode_host, bldp_bslz4_decode_dev,
bldp_bslz4_decode_dev_async + bldp_bslz4_error.  Everything is byte-exact
against tests/bslz4_ref.py, a plain Python statement of the format that shares
nothing with the library or with oracle/ (and is itself checked here against
chunks written by the bitshuffle library, tests/golden/bslz4_v1.npz).

What the corpus pins (bslz4_ref.directed_cases and friends), each at element
sizes 4, 1, 2 and 8 unless it says otherwise:
  * offset x length: offsets 1..256 around the wave width (62..66) and the
    byte/word sizes, match lengths around the offset (overlap on and off), its
    double, the wave width and the 15 / 15 + 255 k length-byte boundaries;
  * literal runs of 0, 1, 14, 15, 16, 269, 270, 271, 525 in mid-block and last;
  * matches that read the previous match's output, that straddle a
    literal/match boundary, four zero-literal matches in a row; a block that
    ends on a match (accepted by host, device and reference alike);
  * blocks of 8 and 64 elements, the largest block the LDS plan admits
    (65488 bytes of dynamic LDS at es = 4) with offsets of `op`, 16385 and
    32000, one block above the plan (es = 4: the host decodes it, the device
    refuses it before any launch);
  * n = 0, tail-only chunks, n around the block and the transpose group;
  * es = 3 through the raw ABI;
  * compressed-buffer residues 0..15, output slots at 4/8/12 mod 16, odd
    slots (es = 1), permuted and gapped slots, untouched bytes around them;
  * one malformed chunk per bounds check, and MUTATIONS single-byte mutations
    (seed bslz4_ref.MUTATION_SEED = 7: 121 accepted = 60.5 %, 79 rejected =
    39.5 % by the reference decoder; both shares are asserted >= 20 %).

Which guard of the current source refuses each malformed chunk.  Read from
lz4_block_host / plan_chunk (host) and k_bslz4 / k_bslz4_plan / describe_chunk
(device) before these ran on a GPU; none of the cases is meant to get past a
guard, every one of them is stopped by a comparison before the index is used:

  case                      host                           device
  offset_0                  off == 0                       k_bslz4: off == 0
  offset_op_plus_1          off > op                       k_bslz4: off > op
  offset_at_op_0            off > op (op = 0)              k_bslz4: off > op
  literals_past_input       ip + lit > slen                k_bslz4: ip + lit > clen
  literals_past_output      op + lit > dcap                k_bslz4: op + lit > nbytes
  match_past_output         op + ml > dcap                 k_bslz4: op + ml > nbytes
  one_byte_long[_match]     op + lit / op + ml > dcap      k_bslz4: the same two
  literal_length_cut        ip >= slen in the lit loop     k_bslz4: ip >= clen (lit loop)
  match_length_cut          ip >= slen in the ml loop      k_bslz4: ip >= clen (ml loop)
  offset_cut                ip + 2 > slen                  k_bslz4: ip + 2 > clen
  one_byte_short            returned length != nb          k_bslz4: op != nbytes
  block_longer_than_bound   op + lit > dcap                k_bslz4_plan: cl > cap
  block_size_overruns       plan_chunk: pos + 4 + cl > len k_bslz4_plan: pos + 4 + cl > end
  trailing_bytes            plan_chunk: pos + tail != len  k_bslz4_plan: pos + tail != end
  tail_one_short            plan_chunk: pos + tail != len  k_bslz4_plan: pos + tail != end
  bytes_not_multiple_of_es  plan_chunk: nb % es            describe_chunk: nb % es (host)
  block_not_multiple_of_8   plan_chunk: (bb / es) % 8      describe_chunk (host)
  block_bytes_0             plan_chunk: bb == 0            describe_chunk (host)

Every index the kernels form is covered by one of these: in[] is read at
ip < clen <= cap only (each ip++ follows an ip < clen or ip >= clen test, the
literal source by ip + lit <= clen, the offset by ip + 2 <= clen); dec[] is
written at op + len <= nbytes <= dcap and read at op - off >= 0; comp[] is read
inside [src, src + len) by the planner's pos + 4 <= end and pos + 4 + cl <= end
and the tail's pos + tail * es == end; out[] is written inside the chunk's slot
because describe_chunk's n * es equals the slot length and the planner's
element counts sum to n; a rejected plan (error bits 2 | 4) stops every
decoding workgroup before it reads the unfinished task table.  A byte mutation
after the header can change only what those comparisons look at.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os
import struct

import numpy as np
import pytest

import bslz4_ref as R
from conftest import GOLDEN

GUARD = 64
FILL = 0xA5
SIZES = (4, 1, 2, 8)


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


# the corpus, built once per process
@functools.lru_cache(maxsize=None)
def directed():
    return tuple(R.directed_cases())


@functools.lru_cache(maxsize=None)
def extras():
    rng = np.random.default_rng(20243)
    return R.es3_case(rng), R.above_plan_case(rng)


@functools.lru_cache(maxsize=None)
def malformed():
    bad, ok = R.malformed_cases()
    return tuple(bad), ok


@functools.lru_cache(maxsize=None)
def mutations():
    return tuple(R.mutation_cases())


def by_size(es):
    return [c for c in directed() if c.es == es]


def named(name):
    return next(c for c in directed() if c.name == name)


def host_decode(pkg, L, chunk: bytes, es: int):
    """bldp_bslz4_decode_host into a buffer of exactly the header's byte count
    (guard bytes around it must survive).  Returns (rc, bytes)."""
    buf = np.frombuffer(bytes(chunk), np.uint8)
    nb, bb = ctypes.c_uint64(), ctypes.c_uint32()
    assert L.bldp_bslz4_info(buf.ctypes.data, buf.size, ctypes.byref(nb), ctypes.byref(bb)) == 0
    assert (nb.value, bb.value) == struct.unpack(">QI", bytes(chunk[:12]))
    out = np.full(nb.value + 2 * GUARD, FILL, np.uint8)
    rc = L.bldp_bslz4_decode_host(buf.ctypes.data, buf.size, es, out.ctypes.data + GUARD,
                                  nb.value)
    assert (out[:GUARD] == FILL).all() and (out[GUARD + nb.value:] == FILL).all(), \
        "the host decoder wrote outside its output"
    return rc, out[GUARD:GUARD + nb.value].tobytes()


# ------------------------------------------------------------------ the reference


def test_reference_bit_planes_by_definition():
    """shuffle / unshuffle against the definition, bit by bit: plane 8 j + k,
    byte g, bit t = bit k of byte j of element 8 g + t."""
    rng = np.random.default_rng(1)
    for es, n in ((1, 8), (2, 16), (3, 24), (4, 40), (8, 16)):
        a = rng.integers(0, 256, (n, es), dtype=np.uint8)
        planes = np.zeros((es * 8, n // 8), np.uint8)
        for e in range(n):
            for j in range(es):
                for k in range(8):
                    planes[8 * j + k, e // 8] |= ((int(a[e, j]) >> k) & 1) << (e % 8)
        assert R.shuffle(a, es) == planes.tobytes()
        assert R.unshuffle(planes.tobytes(), n, es) == a.tobytes()


def test_reference_reads_the_bitshuffle_librarys_chunks():
    """The reference decoder on chunks the bitshuffle library wrote (the
    fixtures up to 64 KiB): it is a statement of the same format."""
    z = np.load(os.path.join(GOLDEN, "bslz4_v1.npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "bslz4_manifest.json")) as f:
        cases = json.load(f)["cases"]
    seen = 0
    for c in cases:
        chunk = z["chunk_" + c["name"]].tobytes()
        if len(chunk) > 65536:
            continue
        assert R.ref_decode_chunk(chunk, 4) == z["raw_" + c["name"]].tobytes(), c["name"]
        seen += 1
    assert seen >= 10


def test_reference_builder_and_decoder_agree():
    """Every block of the corpus: ref_lz4_decode of what SeqBuilder emitted is
    what SeqBuilder tracked (chunk_of asserts it per block); the chunk-level
    reference gives the expected bytes; the greedy compressor round-trips."""
    for c in directed() + extras():
        assert R.ref_decode_chunk(c.chunk, c.es) == c.want, c.name
    rng = np.random.default_rng(2)
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        a = rng.integers(0, 5, 200).astype(dt)
        assert R.ref_decode_chunk(R.encode(a, 64), a.itemsize) == a.tobytes()
        assert R.ref_decode_chunk(R.encode(a, 64, R.lz4_literals), a.itemsize) == a.tobytes()
    sb = R.SeqBuilder().seq(b"abcd", 4, 4)
    assert bytes(sb.block) == b"\x40abcd\x04\x00" and bytes(sb.out) == b"abcdabcd"
    sb = R.SeqBuilder().seq(b"x" * 15, 1, 19 + 255).seq(b"y" * 270)
    assert bytes(sb.block) == (b"\xff\x00" + b"x" * 15 + b"\x01\x00\xff\x00"
                               + b"\xf0\xff\x00" + b"y" * 270)


def test_corpus_covers_what_it_claims():
    """The grid holds every (offset, length) pair the issue lists, with
    overlapping matches at every offset 62..66, and the largest blocks are the
    LDS plan's limit."""
    bound = lambda b: ((b + b // 255 + 16 + 15) & ~15) + ((b + 15) & ~15)  # noqa: E731
    for es in SIZES:
        nb = 512 * es
        for o in R.GRID_OFFSETS:
            c = named(f"grid_o{o}_es{es}")
            want = [m for m in sorted({4, 5, o - 1, o, o + 1, 2 * o, 2 * o + 1, 63, 64, 65, 127,
                                       128, 129, 18, 19, 273, 274, 529})
                    if m >= 4 and o + m <= nb]
            assert R.grid_lengths(o, nb) == want and len(c.want) == len(want) * nb
            if 62 <= o <= 66:
                assert {o - 1, o, o + 1, 2 * o, 2 * o + 1} <= set(want)
        be = R.MAX_BLOCK[es]
        assert bound(be * es) <= 65536 < bound((be + 8) * es)
    assert bound(R.MAX_BLOCK[4] * 4) == 65488 and R.ABOVE_PLAN == R.MAX_BLOCK[4] + 8


# --------------------------------------------------------------- the host decoder


@pytest.mark.parametrize("es", SIZES)
def test_host_decodes_directed_corpus(pkg, L, es):
    """Grid, literal boundaries, chains, a block ending on a match, blocks of 8,
    64 and the largest the LDS plan admits, chunk geometry: byte for byte."""
    cases = by_size(es)
    assert len(cases) >= 30
    for c in cases:
        rc, got = host_decode(pkg, L, c.chunk, es)
        assert rc == 0, (c.name, pkg._lib.last_error())
        assert got == c.want, c.name


def test_host_decodes_block_above_the_lds_plan(pkg, L):
    _, above = extras()
    rc, got = host_decode(pkg, L, above.chunk, 4)
    assert rc == 0 and got == above.want


def test_host_decodes_three_byte_elements(pkg, L):
    """es = 3 through the raw ABI (no dtype has it): block bytes 96 = 4 * 24."""
    c, _ = extras()
    assert struct.unpack(">QI", c.chunk[:12]) == (74 * 3, 96)
    rc, got = host_decode(pkg, L, c.chunk, 3)
    assert rc == 0 and got == c.want


def test_python_wrappers_map_dtypes(pkg):
    """fbh5.bslz4_decode_host at 1-, 2-, 4- and 8-byte dtypes."""
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        c = named(f"n143_es{np.dtype(dt).itemsize}")
        got = pkg.fbh5.bslz4_decode_host(c.chunk, dtype=dt)
        assert got.dtype == dt and got.tobytes() == c.want


def test_host_refuses_malformed_chunks(pkg, L):
    bad, ok = malformed()
    assert len(bad) == 19
    rc, got = host_decode(pkg, L, ok.chunk, 4)
    assert rc == 0 and got == ok.want
    for c in bad:
        with pytest.raises(R.Malformed):
            R.ref_decode_chunk(c.chunk, c.es)
        rc, _ = host_decode(pkg, L, c.chunk, c.es)
        assert rc == pkg._lib.BLDP_EINVAL, c.name


def test_device_entry_refuses_bad_headers_before_launch(pkg, L):
    """Malformed headers and a block above the LDS plan are refused on the host
    by both device entry points, before any HIP call: this runs without a GPU
    (the device pointers are never used)."""
    bad, _ = malformed()
    _, above = extras()
    fake = 1 << 20
    hdr = [c for c in bad if c.where == "header"]
    assert len(hdr) == 3
    for c in hdr + [above]:
        h = np.frombuffer(c.chunk, np.uint8)
        off = np.zeros(1, np.uint64)
        n = np.array([len(c.chunk)], np.uint64)
        olen = np.array([struct.unpack(">Q", c.chunk[:8])[0]], np.uint64)
        for rc in (L.bldp_bslz4_decode_dev(1, h.ctypes.data, fake, off.ctypes.data,
                                           n.ctypes.data, 4, fake, off.ctypes.data,
                                           olen.ctypes.data, None),
                   L.bldp_bslz4_decode_dev_async(1, h.ctypes.data, fake, off.ctypes.data,
                                                 n.ctypes.data, 4, fake, off.ctypes.data,
                                                 olen.ctypes.data, fake, None)):
            assert rc == pkg._lib.BLDP_EINVAL, c.name
            assert ("LDS plan" if c is above else "bad header") in pkg._lib.last_error()


MUTATIONS = 200
MIN_SHARE = 0.2


def test_mutation_shares():
    """Both verdicts are populated (reference decoder alone): seed 7 gives 121
    accepted and 79 rejected of 200."""
    m = mutations()
    acc = sum(c.want is not None for c in m)
    assert len(m) == MUTATIONS
    assert acc >= MIN_SHARE * MUTATIONS and MUTATIONS - acc >= MIN_SHARE * MUTATIONS
    assert (R.MUTATION_SEED, acc) == (7, 121)


def test_host_agrees_with_reference_on_mutations(pkg, L):
    for c in mutations():
        rc, got = host_decode(pkg, L, c.chunk, c.es)
        if c.want is None:
            assert rc == pkg._lib.BLDP_EINVAL, c.name
        else:
            assert rc == 0 and got == c.want, c.name


# -------------------------------------------------------------------------- GPU


def dev_decode(pkg, chunks, es, *, chunk_off=None, slot_off=None, total=None, use_async=False,
               base_align=0):
    """One call of bldp_bslz4_decode_dev (or _async + bldp_bslz4_error) on
    `chunks`, into a buffer of `total` bytes filled with 0xA5.  chunk_off:
    byte offsets in the compressed buffer (default: packed); slot_off: output
    offsets (default: packed after GUARD bytes).  Returns (rc, message, the
    whole output buffer, slot offsets, slot lengths)."""
    import torch

    L, lib = pkg._lib.lib(), pkg._lib
    lens = [len(c) for c in chunks]
    if chunk_off is None:
        chunk_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    chunk_off = np.asarray(chunk_off, np.uint64)
    comp = np.full(int(max(o + n for o, n in zip(chunk_off.tolist(), lens))) + 16, 0x5A, np.uint8)
    for o, c in zip(chunk_off.tolist(), chunks):
        comp[o:o + len(c)] = np.frombuffer(bytes(c), np.uint8)
    olen = np.array([struct.unpack(">Q", bytes(c[:8]))[0] for c in chunks], np.uint64)
    if slot_off is None:
        slot_off = GUARD + np.concatenate([[0], np.cumsum(olen)[:-1]]).astype(np.uint64)
    slot_off = np.asarray(slot_off, np.uint64)
    if total is None:
        total = int((slot_off + olen).max()) + GUARD
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda:0")
    cdev = torch.from_numpy(comp).cuda()
    clen = np.array(lens, np.uint64)
    args = (len(chunks), comp.ctypes.data, cdev.data_ptr(), chunk_off.ctypes.data,
            clen.ctypes.data, es, out.data_ptr(), slot_off.ctypes.data, olen.ctypes.data)
    if use_async:
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = L.bldp_bslz4_decode_dev_async(*args, err.data_ptr(), lib.stream_ptr())
        if rc == 0:
            rc = L.bldp_bslz4_error(err.data_ptr(), lib.stream_ptr())
    else:
        rc = L.bldp_bslz4_decode_dev(*args, lib.stream_ptr())
    msg = lib.last_error() if rc else ""
    torch.cuda.synchronize()
    return rc, msg, out.cpu().numpy(), slot_off.tolist(), olen.tolist()


def assert_slots(out, slot_off, olen, wants, what=""):
    """Every slot holds its chunk's bytes; every byte outside the slots is
    still the fill."""
    outside = np.ones(out.size, bool)
    for k, (o, n, w) in enumerate(zip(slot_off, olen, wants)):
        assert len(w) == n, (what, k)
        assert out[o:o + n].tobytes() == w, (what, k)
        outside[o:o + n] = False
    assert (out[outside] == FILL).all(), (what, "bytes outside the slots were written")


@pytest.mark.gpu
@pytest.mark.parametrize("use_async", [False, True])
@pytest.mark.parametrize("es", SIZES)
def test_gpu_decodes_directed_corpus(pkg, es, use_async):
    """All valid directed chunks of one element size in one launch (the
    65488-byte dynamic-LDS launch among them at es = 4)."""
    cases = by_size(es)
    rc, msg, out, so, ol = dev_decode(pkg, [c.chunk for c in cases], es, use_async=use_async)
    assert rc == 0, msg
    for k, c in enumerate(cases):  # name the chunk that differs
        assert out[so[k]:so[k] + ol[k]].tobytes() == c.want, c.name
    assert_slots(out, so, ol, [c.want for c in cases])


@pytest.mark.gpu
def test_gpu_decodes_three_byte_elements(pkg):
    c, _ = extras()
    rc, msg, out, so, ol = dev_decode(pkg, [c.chunk], 3)
    assert rc == 0, msg
    assert_slots(out, so, ol, [c.want])


@pytest.mark.gpu
def test_gpu_python_wrapper_maps_dtypes(pkg):
    """fbh5.bslz4_decode_dev at 1-, 2-, 4- and 8-byte dtypes."""
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        es = np.dtype(dt).itemsize
        cs = [named(f"n143_es{es}"), named(f"chain_es{es}")]
        got = pkg.fbh5.bslz4_decode_dev([c.chunk for c in cs], dtype=dt, device="cuda:0")
        assert got.element_size() == es
        assert got.cpu().numpy().tobytes() == b"".join(c.want for c in cs)


@pytest.mark.gpu
def test_gpu_mixed_block_sizes_in_one_launch(pkg):
    """Blocks of 8, 64, 512 and 8168 elements in one launch (the LDS plan is
    sized by the largest), with the n = 0 and tail-only chunks between them."""
    names = ["block8_es4", "n0_es4", "largest_es4", "n1_es4", "block64_es4", "n7_es4",
             "grid_o63_es4", "n0_es4", "chain_es4", "block8_es4"]
    cases = [named(n) for n in names]
    assert {c.block_elems for c in cases} == {8, 64, 512, 8168}
    rc, msg, out, so, ol = dev_decode(pkg, [c.chunk for c in cases], 4)
    assert rc == 0, msg
    assert_slots(out, so, ol, [c.want for c in cases])


@pytest.mark.gpu
def test_gpu_refuses_block_above_the_lds_plan(pkg):
    _, above = extras()
    good = named("chain_es4")
    rc, msg, out, _, _ = dev_decode(pkg, [good.chunk, above.chunk], 4)
    assert rc == pkg._lib.BLDP_EINVAL and "LDS plan" in msg
    assert (out == FILL).all()  # refused before any launch


@pytest.mark.gpu
def test_gpu_compressed_buffer_alignment(pkg):
    """The same chunks at every byte residue 0..15 of the compressed buffer."""
    cases = [named("chain_es4"), named("n143_es4"), named("grid_o65_es4")]
    chunks, offs, wants, pos = [], [], [], 0
    for r in range(16):
        for c in cases:
            pos = (pos + 15) // 16 * 16 + r
            offs.append(pos)
            chunks.append(c.chunk)
            wants.append(c.want)
            pos += len(c.chunk)
    rc, msg, out, so, ol = dev_decode(pkg, chunks, 4, chunk_off=offs)
    assert rc == 0, msg
    assert_slots(out, so, ol, wants)


@pytest.mark.gpu
def test_gpu_output_slot_alignment_and_order(pkg):
    """Output slots at 4, 8, 12 mod 16 (es = 4), at odd offsets (es = 1), in
    permuted order with gaps; the bytes between the slots stay untouched."""
    c4 = [named("chain_es4"), named("n143_es4"), named("n9_es4"), named("block8_es4")]
    for res in (4, 8, 12):
        pos, so = GUARD, []
        for c in c4:
            pos = (pos + 15) // 16 * 16 + res
            so.append(pos)
            pos += len(c.want) + 20  # a gap
        rc, msg, out, so, ol = dev_decode(pkg, [c.chunk for c in c4], 4, slot_off=so)
        assert rc == 0, msg
        assert_slots(out, so, ol, [c.want for c in c4], res)
    c1 = [named("chain_es1"), named("n143_es1"), named("n9_es1"), named("block8_es1")]
    pos, so = GUARD, []
    for c in c1:
        pos = (pos + 15) // 16 * 16 + 1 + 2 * (len(so) % 3)  # 1, 3, 5 mod 16
        so.append(pos)
        pos += len(c.want) + 7
    rc, msg, out, so, ol = dev_decode(pkg, [c.chunk for c in c1], 1, slot_off=so)
    assert rc == 0, msg
    assert_slots(out, so, ol, [c.want for c in c1], "odd")
    # permuted and gapped: the slots in the reverse of chunk order, then rotated
    for es, cs in ((4, c4), (1, c1)):
        for order in ([3, 2, 1, 0], [2, 0, 3, 1]):
            pos, place = GUARD, {}
            for k in order:
                place[k] = pos
                pos += (len(cs[k].want) + 36 + 3) // 4 * 4
            so = [place[k] for k in range(4)]
            rc, msg, out, so, ol = dev_decode(pkg, [c.chunk for c in cs], es, slot_off=so)
            assert rc == 0, msg
            assert_slots(out, so, ol, [c.want for c in cs], (es, order))


@pytest.mark.gpu
def test_gpu_refuses_malformed_blocks(pkg):
    """Each malformed block and block table in a call of its own, between two
    good chunks: BLDP_EINVAL, nothing written outside the call's slots, and a
    good chunk decodes afterwards.  (Malformed headers never reach the GPU:
    test_device_entry_refuses_bad_headers_before_launch.)"""
    bad, ok = malformed()
    on_device = [c for c in bad if c.where in ("block", "plan")]
    assert len(on_device) == 16
    for use_async in (False, True):
        for c in on_device:
            rc, msg, out, so, ol = dev_decode(pkg, [ok.chunk, c.chunk, ok.chunk], 4,
                                              use_async=use_async)
            assert rc == pkg._lib.BLDP_EINVAL, (c.name, msg)
            assert ("overruns" in msg) == (c.where == "plan"), (c.name, msg)
            outside = np.ones(out.size, bool)
            for o, n in zip(so, ol):
                outside[o:o + n] = False
            assert (out[outside] == FILL).all(), c.name
            if c.where == "plan":  # a refused block table stops every workgroup
                assert (out == FILL).all(), c.name
        rc, msg, out, so, ol = dev_decode(pkg, [ok.chunk], 4, use_async=use_async)
        assert rc == 0, msg
        assert_slots(out, so, ol, [ok.want])


@pytest.mark.gpu
def test_gpu_agrees_with_host_on_mutations(pkg, L):
    """The same 200 mutations, one call each: the device accepts exactly when
    the host does, and gives the reference's bytes."""
    for c in mutations():
        hrc, _ = host_decode(pkg, L, c.chunk, c.es)
        rc, msg, out, so, ol = dev_decode(pkg, [c.chunk], c.es)
        assert (rc == 0) == (hrc == 0), (c.name, msg)
        if rc == 0:
            assert c.want is not None, c.name
            assert_slots(out, so, ol, [c.want], c.name)
        else:
            assert rc == pkg._lib.BLDP_EINVAL, (c.name, msg)
            assert (out[:GUARD] == FILL).all() and (out[so[0] + ol[0]:] == FILL).all(), c.name
