"""The designed deflate streams of tests/inflatecases.py without a GPU: zlib returns exactly the bytes the writer meant (or raises
where the case says it must), the synchronisation model's claim holds for every case that makes one, and every size a case is
named for is there: token counts, deflate blocks, the bit of the end-of-block code, the code lengths in use.  This is the proof
that the inputs of tests/test_gpu_inflate.py are what their names say; also that the hooks are exported, bound, declared and
documented, and that the constants the cases derive from are the build's."""
import os
import re
import zlib

import pytest

from breakid_amd import abi, capi
from tests import inflatecases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")
HOOKS = ("bk_debug_bgzf_inflate_form", "bk_debug_bgzf_info")
INFO = capi.bgzf_info()
CASES = ic.cases(INFO)
BY = {c.name: c for c in CASES}
LF, DF, PART, CHECK, FULL, RW = (INFO[k] for k in ("LIT_FAST", "DIST_FAST", "LANE_PART_BITS", "LANE_CHECK_BITS", "LANE_FULL_WALKS", "RES_WIN"))


def one(name):
    (s,) = BY[name].streams
    return s


def huffman(s):
    return [k for k, m in enumerate(s.meta) if m["type"]]


def test_hooks_exported_bound_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("Test hooks of the C ABI"):]
    item = item[:item.index("\n* ")]
    for name in HOOKS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in item, name
    assert callable(capi.bgzf_info) and callable(capi.bgzf_inflate_form)
    assert (abi.BGZF_FORM_ROUNDS, abi.BGZF_FORM_SHARED) == (ic.FORM_ROUNDS, ic.FORM_SHARED) == (1, 2)
    assert re.search(r"#define BK_BGZF_FORM_ROUNDS 1\n#define BK_BGZF_FORM_SHARED 2\n", header)
    fuzz = open(os.path.join(ROOT, "tools", "gpu_inflatefuzz.py")).read()
    assert "bgzf_inflate_form" in fuzz


def test_constants_of_the_build():
    assert INFO == ic.TODAY and tuple(INFO) == abi.BGZF_INFO  # (a change of a constant moves the cases with it: update TODAY)
    src = open(os.path.join(CSRC, "bgzf_gpu.hip")).read()
    hdr = open(os.path.join(CSRC, "bgzf_gpu.h")).read()
    assert re.search(r"constexpr int LIT_FAST = %d, DIST_FAST = %d;" % (LF, DF), src)
    assert re.search(r"#define LANE_PART_BITS %d\n#define LANE_CHECK_BITS %d\n" % (PART, CHECK), src)
    assert re.search(r"constexpr int LANE_FULL_WALKS = %d;" % FULL, src) and re.search(r"constexpr uint32_t CHUNK_DW = %d;" % INFO["CHUNK_DW"], src)
    assert re.search(r"constexpr uint32_t RES_WIN = %d;" % RW, src) and re.search(r"constexpr uint32_t RESOLVE_THREADS = %d;" % INFO["RESOLVE_THREADS"], src)
    assert re.search(r"constexpr uint32_t BGZF_BATCH_BLOCKS = %d;" % INFO["BGZF_BATCH_BLOCKS"], hdr)
    assert re.search(r"constexpr uint32_t BGZF_TOKENS_PER_BLOCK = %d;" % INFO["BGZF_TOKENS_PER_BLOCK"], hdr)
    assert re.search(r"constexpr int BGZF_MAX_DEFLATE_BLOCKS = %d;" % INFO["BGZF_MAX_DEFLATE_BLOCKS"], hdr)
    assert "guard < BGZF_MAX_DEFLATE_BLOCKS" in src and not re.search(r"guard < \d", src)
    # the cases move with the constants
    other = dict(INFO, LANE_FULL_WALKS=FULL - 2, RES_WIN=RW // 2, BGZF_MAX_DEFLATE_BLOCKS=1000)
    names = {c.name for c in ic.cases(other)}
    assert {"1000_deflate_blocks", "1001_deflate_blocks", "isize_%d" % (RW // 2 + 1), "match_of_258_starting_1_before_the_resolve_window_edge"} <= names
    assert any(re.search(r"window_0_long_passes_%d_to_the_rounds" % (FULL - 1), n) for n in names)


def test_the_writer_itself():
    """the writer's tables, its canonical codes and its run-length coder; a stream of all three block kinds inflates to what was meant"""
    assert ic.LEN_BASE[-1] == 258 and len(ic.LEN_BASE) == len(ic.LEN_EXTRA) == 29 and len(ic.DIST_BASE) == len(ic.DIST_EXTRA) == 30
    assert all(ic.LEN_BASE[k] + (1 << ic.LEN_EXTRA[k]) == ic.LEN_BASE[k + 1] for k in range(27)) and ic.LEN_BASE[27] + 31 == 258
    assert all(ic.DIST_BASE[k] + (1 << ic.DIST_EXTRA[k]) == ic.DIST_BASE[k + 1] for k in range(29)) and ic.DIST_BASE[29] + (1 << 13) - 1 == 32768
    assert ic.canon_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]  # RFC 1951 3.2.2
    assert ic.kraft(ic.FIXED_LL) == 32768 and ic.kraft(ic.FIXED_DL) == 32768
    for k in (2, 3, 19, 30, 257, 286):
        assert ic.kraft(ic.complete_lengths(k)) == 32768 and len(ic.complete_lengths(k)) == k
    for seq in ([0] * 300, [3] * 7 + [0] * 2 + [5] + [0] * 150 + [4, 4, 4, 4], [1, 2, 3, 3]):
        assert ic.rle_expand(ic.rle_greedy(seq)) == seq and ic.rle_expand(ic.rle_plain(seq)) == seq
    text = ic.lcg_bytes(700, 1, 65, 70) + b"ACGT" * 100
    d = ic.Deflate().stored(text[:100]).fixed(list(text[100:300]) + [(100, 50), ic.EOB]).dynamic(list(text[400:]) + [(258, 1), ic.EOB], ic.complete_lengths(286), ic.complete_lengths(30),
                                                                                                 final=True, rle="greedy")
    assert zlib.decompress(d.bytes(), -15) == bytes(d.out) == text[:300] + text[250:300] * 2 + text[400:] + text[-1:] * 258


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_zlib_on_every_case(case):
    assert case.cls in ("A", "B", "D") and case.streams
    for s in case.streams:
        ref, why = ic.zlib_reference(s), ic.zlib_error(s)
        if case.cls in ("A", "D"):
            assert ref is not None, why
            assert ref == s.intended and len(ref) == s.isize and 0 < s.isize <= 65536
        else:
            assert ref is None or len(ref) != s.isize  # zlib raises, or the stream does not give the bytes its block promises
            assert (ref is None) == (s.intended is None)
        assert len(s.data) <= ic.BGZF_MAX_STREAM


def test_classes():
    cls = {k: [c for c in CASES if c.cls == k] for k in "ABCD"}
    assert not cls["C"] and [c.name for c in cls["D"]] == ["%d_deflate_blocks" % (INFO["BGZF_MAX_DEFLATE_BLOCKS"] + 1)]
    assert {c.family for c in cls["A"]} == set(ic.FAMILIES) and {c.family for c in cls["B"]} <= {"invalid", "extras"}
    # what zlib says about the sets that once were class C, and about its one exception
    assert "invalid literal/lengths set" in ic.zlib_error(one("incomplete_literal_length_set"))
    assert "invalid distances set" in ic.zlib_error(one("incomplete_distance_set"))
    assert "invalid code lengths set" in ic.zlib_error(one("incomplete_code_length_code"))
    for name in ("incomplete_literal_length_set", "incomplete_distance_set"):
        s = one(name)
        m = s.meta[1]
        assert ic.kraft(m["ll" if "literal" in name else "dl"]) < 32768 and ic.kraft(m["dl" if "literal" in name else "ll"]) in (0, 32768)
        assert all(m["ll"][x.lsym] and (x.dsym is None or m["dl"][x.dsym]) for x in m["syms"])  # assigned codes only
    assert BY["lone_1_bit_distance_code"].cls == "A" and one("lone_1_bit_distance_code").meta[0]["dl"][:2] == [1, 0]
    m = one("literal_length_set_of_a_1_bit_end_of_block_alone").meta[1]
    assert [l for l in m["ll"] if l] == [1] and m["ll"][256] == 1
    assert BY["extras_284_with_extra_31"].cls == "A"  # zlib takes 284 + 31 for 258


def test_code_lengths_in_use():
    for variant, name in enumerate(("long_codes_eob_short", "long_codes_eob_all_ones_15")):
        s = one(name)
        m = s.meta[1]
        ll, dl = m["ll"], m["dl"]
        assert ic.kraft(ll) == 32768 and ic.kraft(dl) == 32768 and max(ll) == 15 and max(dl) == 15
        codes, dcodes = ic.canon_codes(ll), ic.canon_codes(dl)
        used = {(x.lsym, x.kind) for x in m["syms"]}
        dused = {x.dsym for x in m["syms"] if x.kind == "match"}
        for L in (LF, LF + 1, 15):
            syms = [k for k in range(288) if ll[k] == L]
            assert len(syms) >= 2 and (syms[0], "lit") in used and ((syms[-1], "match") in used or syms[-1] == ic.EOB), (name, L)  # first and last code of the length
        for L in (DF, DF + 1, 15):
            syms = [k for k in range(32) if dl[k] == L]
            assert len(syms) >= 2 and syms[0] in dused and syms[-1] in dused, (name, L)
        last15 = max(k for k in range(288) if ll[k] == 15)
        assert codes[last15] == 0x7FFF and dcodes[max(k for k in range(32) if dl[k] == 15)] == 0x7FFF  # the all-ones codes of complete sets
        assert (last15 == ic.EOB) == (variant == 1) and (ll[ic.EOB] <= LF) == (variant == 0)
        # the rounds meet every long literal/length code at the head of a round and later in one; every long distance code, and a long
        # length code in front of a long distance code, on the scalar path
        where = ic.rounds_model(s, 1, INFO)
        for L in (LF, LF + 1, 15):
            for kind in ("lit", "match"):
                if variant == 1 and L == 15 and kind == "match":
                    continue  # the end-of-block code is the last 15-bit code there: no length symbol can follow it
                got = {w for x, w in where if x.lcode_len == L and x.kind == kind}
                assert {"head", "mid"} <= got, (name, L, kind, got)
        for L in (DF + 1, 15):
            assert [1 for x, w in where if x.kind == "match" and x.dcode_len == L and w == "scalar"], (name, L)
            assert [1 for x, w in where if x.kind == "match" and x.dcode_len == L and x.lcode_len > LF and w == "scalar"], (name, L)
        assert not [1 for x, w in where if w == "scalar" and x.dcode_len <= DF]
        if variant == 1:
            assert where[-1][0].kind == "eob" and where[-1][0].lcode_len == 15
        # the lanes: a code of every long length lies across a checkpoint of the first window, as a literal/length or a distance code
        wins = ic.sync_model(s, 1, INFO)
        assert not any(w["rounds"] for w in wins)
        cps = [m["first_bit"] + i * PART + CHECK for i in range(64) if m["first_bit"] + i * PART + CHECK < m["eob_bit"]]
        assert len(cps) >= 8
        under_l = {x.lcode_len for x in m["syms"] for c in cps if x.bit <= c < x.bit + x.lcode_len}
        under_d = {x.dcode_len for x in m["syms"] if x.kind == "match" for c in cps if x.bit + x.lbits <= c < x.bit + x.lbits + x.dcode_len}
        assert {LF, LF + 1, 15} <= under_l | under_d and (under_l & {LF + 1, 15}) and (under_d & {DF + 1, 15}), (name, under_l, under_d)


def test_extra_bits_and_distances():
    for name in ("extras_fixed_dist32768_at_32768_into_stored", "extras_dynamic_hlit286_hdist30"):
        s = one(name)
        m = s.meta[1]
        got_l = {(x.lsym, x.lbits - x.lcode_len) for x in m["syms"] if x.kind == "match"}
        assert {x for x, _ in got_l} == set(range(257, 286))
        first = m["syms"][0]
        assert first.opos == 32768 and first.dsym == 29 and s.meta[0]["type"] == 0 and len(s.intended) > 32768 + 258
        assert s.intended[32768:32768 + 258] == s.intended[:258]  # distance 32768 at output position 32768, into the stored block
        assert {x.dsym for x in m["syms"] if x.kind == "match"} == set(range(30))
    # minimum and maximum extra value of every code: re-read from the bits
    s = one("extras_fixed_dist32768_at_32768_into_stored")
    bits = ic._Bits(s.data)
    seen_l, seen_d = set(), set()
    for x in s.meta[1]["syms"]:
        if x.kind == "match":
            nb = ic.LEN_EXTRA[x.lsym - 257]
            seen_l.add((x.lsym, (bits.peek(x.bit + x.lcode_len) & ((1 << nb) - 1)) if nb else 0))
            nb = ic.DIST_EXTRA[x.dsym]
            seen_d.add((x.dsym, (bits.peek(x.bit + x.lbits + x.dcode_len) & ((1 << nb) - 1)) if nb else 0))
    assert all({(k, 0), (k, (1 << ic.LEN_EXTRA[k - 257]) - 1)} <= seen_l for k in range(257, 286))
    assert all({(k, 0), (k, (1 << ic.DIST_EXTRA[k]) - 1)} <= seen_d for k in range(30))
    m = one("extras_dynamic_hlit286_hdist30").meta[1]
    assert (m["hlit"], m["hdist"]) == (286, 30)


def test_header_forms():
    m = one("hlit257_hdist1_one_zero_distance_length").meta[0]
    assert (m["hlit"], m["hdist"], m["dl"][0]) == (257, 1, 0) and m["ntok"] == 0
    m = one("hclen5_the_smallest_that_can_name_a_code").meta[0]
    assert m["hclen"] == 5 and sorted(l for l in m["ll"] if l) == [8] * 256
    m = one("hclen19_every_code_length_code_4_bits").meta[1]
    assert m["hclen"] == 19 and m["cl_lens"] == [4] * 16 + [0] * 3
    m = one("hclen4_can_name_no_code").meta[1]
    assert m["hclen"] == 4 and "missing end-of-block" in ic.zlib_error(one("hclen4_can_name_no_code"))
    m = one("code16_repeats_across_the_literal_distance_boundary").meta[1]
    assert m["rle"][-2:] == [(2,), (16, 4)] and m["hlit"] == 257 and m["hdist"] == 4 and m["ll"][256] == 2 and m["dl"][:4] == [2, 2, 2, 2]
    m = one("code18_with_138").meta[0]
    assert (18, 138) in m["rle"]
    s = one("fixed_directly_after_dynamic_then_dynamic")
    assert [b["type"] for b in s.meta] == [2, 1, 2]
    s = one("literal_length_set_of_a_1_bit_end_of_block_alone")
    assert [b["type"] for b in s.meta] == [0, 2] and [x.kind for x in s.meta[1]["syms"]] == ["eob"]


def test_stored_blocks():
    s = one("stored_len_0_and_1")
    assert [b["end_bit"] - b["first_bit"] for b in s.meta if b["type"] == 0] == [0, 8, 0]
    (name,) = [n for n in BY if n.startswith("stored_len_") and n.endswith("_the_longest_a_bgzf_block_holds")]
    assert len(one(name).data) == ic.BGZF_MAX_STREAM == 65510 and one(name).isize == 65505  # a stored block of 65535 bytes does not fit a BGZF block
    for endbit, name in ((5, "stored_after_huffman_block_ending_at_bit_5_no_padding"), (6, "stored_after_huffman_block_ending_at_bit_6")):
        s = one(name)
        assert s.meta[0]["end_bit"] % 8 == endbit and s.meta[1]["type"] == 0 and s.meta[1]["hdr_bit"] == s.meta[0]["end_bit"]
        assert (s.meta[1]["hdr_bit"] + 3) % 8 == (0 if endbit == 5 else 1)  # bit 5: the three header bits end on the byte boundary
        assert s.meta[1]["first_bit"] == (s.meta[1]["hdr_bit"] + 3 + 7) // 8 * 8 + 32
    C = INFO["CHUNK_DW"]
    seen = set()
    for c in CASES:
        g = re.match(r"stored_then_header_(\d+)_dwords_ahead_in_off_(\d)", c.name)
        if g:
            s = c.streams[0]
            ahead, al = int(g.group(1)), int(g.group(2))
            assert s.in_align == al and (8 * al + s.meta[1]["hdr_bit"]) >> 5 == ahead and s.meta[1]["type"] == 1
            seen.add((ahead, al))
    assert {(C - 1, 0), (C, 0), (2 * C - 1, 0), (2 * C, 0), (C, 1), (C, 2), (C, 3)} == seen
    # the image gives every stream the alignment it asks for
    streams = [s for c in CASES if c.family == "stored" and c.cls == "A" for s in c.streams]
    _, offs = ic.bgzf_image(streams)
    assert all(s.in_align is None or off & 3 == s.in_align for s, off in zip(streams, offs))


def test_sizes():
    for isize in (65533, 65534, 65535, 65536, RW - 3, RW - 2, RW - 1, RW + 1, RW + 2, RW + 3, 2 * RW + 1):
        s = one("isize_%d" % isize)
        last = s.meta[-1]["syms"][-2]
        assert s.isize == isize and last.kind == "match" and s.meta[-1]["ntok"] > 40  # the last bytes are copied ones
    s = one("one_literal_and_21845_matches_of_3")
    assert s.meta[0]["ntok"] == 21845 == INFO["BGZF_TOKENS_PER_BLOCK"] - 1 and s.isize == 65536 and [x.kind for x in s.meta[0]["syms"][:2]] == ["lit", "match"]
    n = INFO["BGZF_MAX_DEFLATE_BLOCKS"]
    assert len(one("%d_deflate_blocks" % n).meta) == n and len(one("%d_deflate_blocks" % (n + 1)).meta) == n + 1
    assert BY["%d_deflate_blocks" % n].cls == "A" and BY["%d_deflate_blocks" % (n + 1)].cls == "D"
    # abutting blocks (out_align 1): blocks with copies start at every out_off & 3
    seen = set()
    for fam in ic.FAMILIES:
        off = 0
        for c in CASES:
            if c.cls == "A" and c.family == fam:
                for s in c.streams:
                    if sum(b["ntok"] for b in s.meta):
                        seen.add(off & 3)
                    off += s.isize
    assert seen == {0, 1, 2, 3}


def test_lanes_geometry():
    W = 64 * PART
    for at in (W - 1, W, W + 1):
        s = one("end_of_block_code_at_bit_%d" % at)
        m = s.meta[0]
        assert m["eob_bit"] - m["first_bit"] == at and m["type"] == 1
        wins = ic.sync_model(s, 0, INFO)
        assert len(wins) == (1 if at < W else 2) and not any(w["rounds"] for w in wins)
    s = one("stream_ends_inside_lane_0")
    assert 8 * len(s.data) < PART
    for delta in (-1, 0, 1):
        s = one("length_code_ends_%+d_bits_from_a_part_boundary" % delta)
        m = s.meta[0]
        (x,) = [x for x in m["syms"] if x.kind == "match"]
        assert x.bit + x.lbits - m["first_bit"] == 3 * PART + delta and x.lbits == x.lcode_len == 7  # the distance code starts there
    s = one("three_windows")
    wins = ic.sync_model(s, 0, INFO)
    assert len(wins) == 3 and not any(w["rounds"] for w in wins) and s.meta[0]["ntok"] > 5


def test_synchronisation_claims():
    s = one("every_code_8_bits_every_part_starts_on_a_code")
    assert PART % 8 == 0 and ic.sync_model(s, 0, INFO) == [{"passes": 1, "long": 1, "rounds": False}]  # on the code grid from the start
    assert sorted(l for l in s.meta[0]["ll"] if l) == [8] * 256
    stays, leaves_later, both_sides = 0, 0, set()
    for c in CASES:
        if c.family != "sync" or c.name.startswith("every_code"):
            continue
        wins = ic.sync_model(c.streams[0], 0, INFO)
        tail = "_long_passes_" + "_".join(str(w["long"]) for w in wins) + ("_to_the_rounds" if wins[-1]["rounds"] else "")
        assert c.name.endswith(tail), (c.name, wins)  # the model's pass counts are in the name
        assert all(w["long"] <= FULL for w in wins[:-1]) and (wins[-1]["long"] == FULL + 1) == wins[-1]["rounds"]
        stays += any(not w["rounds"] and w["long"] >= 2 for w in wins)
        leaves_later += len(wins) > 1 and wins[-1]["rounds"]
        g = re.match(r"unsynchronised_stretch_of_(\d+)_parts_in_window_(\d)", c.name)
        if g:
            both_sides.add((int(g.group(2)), wins[-1]["rounds"], wins[-1]["long"]))
            assert len(wins) == int(g.group(2)) + 1
    assert stays >= 2 and leaves_later >= 2
    for w in (0, 1):
        assert (w, False, FULL) in both_sides and (w, True, FULL + 1) in both_sides and (w, False, FULL - 1) in both_sides
    # the window that goes to the rounds with codes above both direct tables inside it
    for w in (0, 1):
        (c,) = [c for c in CASES if c.name.startswith("unsynchronised_stretch_of_15_bit_length_and_distance_codes_in_window_%d" % w)]
        s = c.streams[0]
        wins = ic.sync_model(s, 0, INFO)
        m = s.meta[0]
        assert len(wins) == w + 1 and wins[-1]["rounds"] and ic.kraft(m["ll"]) == 32768 == ic.kraft(m["dl"])
        run = [x for x in m["syms"] if x.kind == "match"]
        assert len(run) >= (FULL + 3) * PART // 31 and all(x.lcode_len == 15 > LF and x.dcode_len == 15 > DF and x.lbits + x.dbits == 31 for x in run)
        bits = ic._Bits(s.data)
        assert bits.peek(run[0].bit) & 0x7FFFFFFF == 0x7FFFFFFF  # one bits: a walk from a wrong bit reads the same code again
        assert run[0].bit - m["first_bit"] >= w * 64 * PART and (run[-1].bit - m["first_bit"]) // (64 * PART) == w
        if w:
            assert run[0].bit > m["first_bit"] + 64 * PART  # literals and tokens of the first window were written by the lanes before


def test_resolve_edges():
    for back in (1, 257, 258):
        s = one("match_of_258_starting_%d_before_the_resolve_window_edge" % back)
        x = s.meta[1]["syms"][0]
        assert x.kind == "match" and x.opos == RW - back and x.lbits - x.lcode_len == 0 and x.lsym == 285
    s = one("match_source_wholly_in_an_earlier_window")
    x = s.meta[1]["syms"][0]
    assert x.opos >= RW and x.opos - RW + 258 <= RW and s.intended[x.opos:x.opos + 258] == s.intended[x.opos - RW:x.opos - RW + 258]
    s = one("distance_1_run_across_four_windows")
    assert s.isize == 4 * RW == 65536 and s.intended == bytes([33]) * 65536
    s = one("chain_of_matches_each_copying_the_one_before")
    assert s.meta[0]["ntok"] >= 7000 and s.intended[:21000] == bytes([1, 2, 3]) * 7000
    s = one("resolve_window_with_no_token_starting_in_it")
    starts = {x.opos // RW for b in s.meta if b["type"] for x in b["syms"] if x.kind == "match"}
    assert starts == {0, 2} and s.isize > 2 * RW


def test_batch_image():
    img, streams = ic.batch_image(INFO)
    n = INFO["BGZF_BATCH_BLOCKS"] + 1
    assert len(streams) == n and [i for i, s in enumerate(streams) if s.isize > 1] == [n - 3, n - 2, n - 1]
    assert all(ic.zlib_reference(s) == s.intended for s in streams[:300] + streams[-4:])
    assert ic.bgzf_scratch_bytes(n, INFO) > 2.8e9
