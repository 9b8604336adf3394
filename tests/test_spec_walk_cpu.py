"""tests/spec_ref.py, the host mirror of the shape-specialised kernels' template choice, held on the CPU: against the library's
SOURCES (every `using S... = Shape3<...>` line, spec_match's candidate table and padding rule, the sub-chunk threshold, the text of
the Shape3 members the mirror restates, t4_merge_dims' limits), and -- the condition that keeps tests/test_spec_walk_gpu.py
honest -- its case table against the mirror: every template with a sub-chunk walk is named exact, padded and under four cores,
every geometry of the table maps onto the template and pad flag the table claims, and the one template whose walk re-stages its
core-1 block (MULTI && !B1ONCE) is flagged.  A template that gains Shape3::SUB fails here until the table names it."""
import os
import re

import spec_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


SPEC, TT, COMMON, INTERNAL = _read("ttx_tt_spec.inc"), _read("ttx_tt.hip"), _read("ttx_tt_common.h"), _read("ttx_internal.h")


def _define(src, name):
    m = re.findall(rf"^#define {name} (\d+)\s*$", src, flags=re.M)
    assert len(m) == 1, f"{name}: {len(m)} definitions"
    return int(m[0])


def _const(src, name):
    m = re.findall(rf"constexpr (?:int|long long) {name} = (\d+);", src)
    assert len(m) == 1, f"{name}: {len(m)} definitions"
    return int(m[0])


def _word(x):
    x = x.strip()
    return int(x) if x.isdigit() else x


def test_constants_are_the_sources():
    assert _const(COMMON, "kThreads") // _const(INTERNAL, "kWave") == SR.K_WAVES and "kWaves = kThreads / kWave;" in COMMON
    assert _define(SPEC, "TTX_NP32") == SR.TTX_NP32 and _define(SPEC, "TTX_MC32") == SR.TTX_MC32 and _define(SPEC, "TTX_BFS") == SR.TTX_BFS
    assert _const(SPEC, "kMaxPadWaste") == SR.MAX_PAD_WASTE
    assert _define(TT, "TTX_SUBCHUNK_NNZ") == SR.SUBCHUNK_NNZ and _define(TT, "TTX_SUBCHUNKS") == SR.SUBCHUNKS
    assert _const(TT, "kT4Slice") == SR.T4_SLICE and _const(TT, "kT4Stage") == SR.T4_STAGE
    # the chunk length: sub-chunks at a large batch or under the test library's knob, and only where the shape has them
    assert "const int ks = (nnz >= TTX_SUBCHUNK_NNZ || g_chunk_override == 64) ? TTX_SUBCHUNKS : 1;" in TT
    assert "constexpr int mc_of(int ks) { return S::MC * (S::SUB ? ks : 1); }" in TT
    assert "if (P.MC > S::MC)" in SPEC  # (what makes a launch take the MULTI variants)


def test_shape3_members_are_the_mirrored_text():
    m = re.search(r"template <int R1_, int Q1_, int R2_, int Q2_, int NP_ = (\d+), int MC_ = (\d+), int Q0_ = (\d+)>\s*struct Shape3 \{", SPEC)
    assert m and [int(x) for x in m.groups()] == [1, 32, 4], "the defaults of Shape3's template arguments"
    body = SPEC[m.end():SPEC.index("};", m.end())]
    for name, text in SR.EXPR.items():
        assert len(re.findall(rf"\b{name} = {re.escape(text)}[,;]", body)) == 1, f"Shape3::{name} is no longer `{text}`"
    assert "NP = NP_, MC = MC_;" in body and "Q0 = Q0_, R1 = R1_, Q1 = Q1_, R2 = R2_, Q2 = Q2_;" in body


def test_every_template_line_is_mirrored():
    found = {name: tuple(_word(x) for x in args.split(",")) for name, args in re.findall(r"^using (S2?_[0-9_]+) = Shape3<([^>]*)>;", SPEC, flags=re.M)}
    assert found == SR.TEMPLATES
    # ... and a few of the derived members by hand
    s = SR.SHAPES
    assert (s["S_32_4_32_4"].NP, s["S_32_4_32_4"].MC, s["S_32_4_32_4"].LPG, s["S_32_4_32_4"].BFS) == (2, 16, 4, True)
    assert (s["S2_16_4_16_4"].NP, s["S2_16_4_16_4"].MC, s["S2_16_4_16_4"].LPG, s["S2_16_4_16_4"].Q0) == (1, 32, 8, 2)
    assert (s["S_32_8_32_8"].N1, s["S_32_8_32_8"].LDBF, s["S_32_8_32_8"].K0P * s["S_32_8_32_8"].LDBF) == (256, 258, 8256)
    assert not s["S_16_8_16_8"].COOP and not s["S2_16_2_16_4"].COOP and not s["S_64_4_64_4"].SUB_ and not s["S_32_8_32_16"].SUB_


def _id_to_template(x):
    x = x.strip()
    return None if x == "SPEC_NONE" else re.sub(r"^SPEC", "S", x)


def test_candidate_table_and_padding_rule_are_the_sources():
    m = re.search(r"static const Cand cands\[\] = \{(.*?)\n  \};", SPEC, flags=re.S)
    assert m
    rows = re.findall(r"\{(\d+), (\d+), (\d+), \{([^}]*)\}\}", m.group(1))
    got = [(int(a), int(b), int(c), tuple(_id_to_template(x) for x in ids.split(","))) for a, b, c, ids in rows]
    assert got == SR.CANDS
    assert all(t is None or t in SR.TEMPLATES for row in got for t in row[3])
    L = SR.MATCH_LIMITS
    assert f"if (q0 > {L['q0']} || q1 > {L['q1']} || q2 > {L['q2']} || r1 > {L['r']} || r2 > {L['r']}) return SPEC_NONE;" in SPEC
    assert "const int R = rmax <= 16 ? 16 : (rmax <= 32 ? 32 : (rmax <= 64 ? 64 : 128));" in SPEC
    assert "if (q0 > c.Q0 || q1 > c.Q1 || q2 > c.Q2 || c.id[ri] == SPEC_NONE) continue;" in SPEC
    assert "const bool exact = q0 == c.Q0 && q1 == c.Q1 && q2 == c.Q2 && r1 == R && r2 == R;" in SPEC
    assert "const long long real = (long long)q0 * r1 * q1 * r2 + (long long)q0 * q1 * r2 * q2;" in SPEC
    assert "const long long padded = (long long)c.Q0 * R * c.Q1 * R + (long long)c.Q0 * c.Q1 * R * c.Q2;" in SPEC
    assert "if (real * kMaxPadWaste < padded) return SPEC_NONE;" in SPEC
    assert "if (g_disable_pad) return SPEC_NONE;" in SPEC  # (ttx_debug_skip bit 15: spec_match(exact_only=True))
    # every template is dispatched by exactly one candidate
    named = [t for row in SR.CANDS for t in row[3] if t]
    assert sorted(named) == sorted(SR.TEMPLATES)
    # four cores on the three-core kernels
    sq = re.sub(r"\s+", "", TT)
    assert ("if(d.T!=4||g_disable_spec||(longlong)d.q[2]*d.q[3]>32||d.q[3]>8||(longlong)d.r[2]*d.q[2]*d.r[3]>kT4Slice||d.r[3]>128||"
            "(longlong)d.r[2]*d.q[2]*d.q[3]+(longlong)d.r[3]*d.q[3]>kT4Stage)returnfalse;") in sq
    assert "e.q[2]=d.q[2]*d.q[3];" in sq and "if(!spec_match(e))returnfalse;" in sq


def test_spec_match_on_hand_written_geometries():
    assert SR.spec_match([4, 4, 4], [32, 32]) == ("S_32_4_32_4", False)
    assert SR.spec_match([4, 4, 4], [32, 16]) == ("S_32_4_32_4", True)
    assert SR.spec_match([3, 4, 5], [13, 12]) == ("S_16_4_16_8", True) and SR.spec_match([3, 4, 5], [13, 12], exact_only=True) == (None, False)
    assert SR.spec_match([2, 2, 4], [16, 16]) == ("S2_16_2_16_4", False)
    assert SR.spec_match([1, 1, 3], [2, 2]) == (None, False)           # less than an eighth of the smallest template
    assert SR.spec_match([5, 4, 4], [16, 16]) == (None, False) and SR.spec_match([4, 4, 4], [129, 16]) == (None, False)
    assert SR.spec_match([4, 8, 32], [64, 64]) == (None, False)        # (no template at that rank)
    assert SR.spec_match([4, 4, 8], [40, 64]) == ("S_64_4_64_8", True)
    assert SR.t4_merged([4, 8, 4, 2], [32, 32, 8]) == ([4, 8, 8], [32, 32]) and SR.t4_merged([2, 4, 4, 4], [32, 32, 32]) == ([2, 4, 16], [32, 32])
    assert SR.t4_merged([4, 4, 4, 16], [16, 16, 16]) is None and SR.t4_merged([4, 4, 8, 8], [16, 16, 16]) is None
    assert SR.t4_merged([4, 4, 4, 2], [64, 64, 64]) is None             # (a core-2 slice beyond kT4Slice)
    assert SR.spec_mc([4, 4, 4], [32, 32], 1000) == 16 and SR.spec_mc([4, 4, 4], [32, 32], 131072) == 64 and SR.spec_mc([4, 4, 4], [32, 32], 131071) == 16
    assert SR.spec_mc([2, 4, 4], [16, 16], 10, knob64=True) == 128 and SR.spec_mc([4, 4, 4], [64, 64], 10 ** 6) == 16
    assert SR.spec_mc([4, 8, 4, 2], [32, 32, 8], 10, knob64=True) == 64 and SR.spec_mc([5, 3, 4], [8, 12], 10) == 0


def test_the_templates_with_a_walk_are_the_eight_of_the_case_table():
    sub = sorted(name for name, s in SR.SHAPES.items() if s.SUB)
    assert sub == sorted(SR.SUB_TEMPLATES) and len(sub) == 8, "a template gained or lost Shape3::SUB: name it in spec_ref's case table"
    assert tuple(n for n in SR.SUB_TEMPLATES if not SR.SHAPES[n].B1ONCE) == SR.NOT_B1ONCE == ("S_32_8_32_8",)
    for name in SR.SUB_TEMPLATES:
        s = SR.SHAPES[name]
        assert s.COOP and s.MC % (s.LPG * SR.K_WAVES) == 0
        # the counts: sub-chunk and chunk boundaries, a last group that is not whole, at most about 300 lookups
        M = s.MC
        assert SR.walk_counts(name) == [M + 1, 2 * M, 3 * M - 1, 4 * M, 4 * M + 1, 9 * M + s.LPG + 1]
        assert (3 * M - 1) % s.LPG != 0 and max(SR.walk_counts(name)) <= 300


def test_case_table_names_every_walk_in_every_form():
    for name in SR.SUB_TEMPLATES:
        s = SR.SHAPES[name]
        q, ranks = SR.EXACT[name]
        assert SR.spec_match(q, ranks) == (name, False), f"{name} exact"
        assert SR.spec_mc(q, ranks, 100) == s.MC and SR.spec_mc(q, ranks, 100, knob64=True) == SR.SUBCHUNKS * s.MC
        assert SR.spec_mc(q, ranks, SR.SUBCHUNK_NNZ) == SR.SUBCHUNKS * s.MC
        q, ranks = SR.PADDED[name]
        assert SR.spec_match(q, ranks) == (name, True), f"{name} padded: {SR.spec_match(q, ranks)}"
        assert SR.spec_match(q, ranks, exact_only=True) == (None, False)
        assert SR.spec_mc(q, ranks, 100, knob64=True) == SR.SUBCHUNKS * s.MC
        assert int(q[0] * q[1] * q[2]) <= 256
        if SR.four_core_reachable(name):
            assert name in SR.FOUR_CORES, f"{name}: a four-core geometry can merge onto it and the table has none"
    assert all(SR.four_core_reachable(n) for n in SR.SUB_TEMPLATES) and sorted(SR.FOUR_CORES) == sorted(SR.SUB_TEMPLATES)
    for name, (q, ranks) in SR.FOUR_CORES.items():
        m = SR.t4_merged(q, ranks)
        assert m is not None and SR.spec_match(*m) == (name, False), f"{name} under four cores: {m}"
        assert SR.match_any(q, ranks) == (name, False) and SR.spec_mc(q, ranks, 100, knob64=True) == SR.SUBCHUNKS * SR.SHAPES[name].MC
    # the two four-core geometries the walk's MFMA / VALU helpers are named for
    assert SR.FOUR_CORES["S_32_8_32_8"] == ([4, 8, 4, 2], [32, 32, 8]) and SR.FOUR_CORES["S2_32_4_32_4"] == ([2, 4, 2, 2], [32, 32, 16])
    assert len(SR.P3) == 3 and len(SR.P4) == 4
    # the extra cases: the template without B1ONCE and one with it
    assert SR.EXTRA_TEMPLATES[0] in SR.NOT_B1ONCE and SR.SHAPES[SR.EXTRA_TEMPLATES[1]].B1ONCE
    assert all(n in SR.SUB_TEMPLATES for n in SR.EXTRA_TEMPLATES)
    assert SR.EXTRA_KINDS == ("weights", "live", "three_tables", "all_slices")


def test_padded_geometries_clear_every_vector_bit_somewhere():
    """RealDims::v4: bit 0 / 1 / 2 = r1 / r2 / q2 is a multiple of 4; and an output row that is no multiple of 4 floats"""
    geoms = list(SR.PADDED.values())
    assert any(r[0] % 4 for _, r in geoms) and any(r[1] % 4 for _, r in geoms) and any(q[2] % 4 for q, _ in geoms)
    assert any((q[0] * q[1] * q[2]) % 4 for q, _ in geoms)
    # ... and one that keeps them all (the padded variants' float4 paths)
    assert any(r[0] % 4 == 0 and r[1] % 4 == 0 and q[2] % 4 == 0 for q, r in geoms)
