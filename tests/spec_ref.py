"""A host mirror of the shape-specialised kernels' template choice (csrc/ttx_tt_spec.inc: Shape3, spec_match; csrc/ttx_tt.hip:
spec_mc, t4_merge_dims) and the case table of tests/test_spec_walk_gpu.py.  TEST INFRASTRUCTURE: plain Python, no device.
tests/test_spec_walk_cpu.py reads the sources and fails when a template, the candidate table or one of the mirrored expressions
changes without this file.

The sub-chunk walk: from SUBCHUNK_NNZ lookups per launch (or, in the test library, under ttx_set_chunk(64)) a template with
Shape3::SUB is planned with chunks of SUBCHUNKS sub-chunks of Shape3::MC lookups and runs its MULTI kernel variant."""

K_WAVES = 4          # kWaves = kThreads / kWave (csrc/ttx_tt_common.h)
TTX_NP32 = 2         # csrc/ttx_tt_spec.inc
TTX_MC32 = 16
TTX_BFS = 1
MAX_PAD_WASTE = 8    # kMaxPadWaste
SUBCHUNK_NNZ = 131072  # TTX_SUBCHUNK_NNZ (csrc/ttx_tt.hip)
SUBCHUNKS = 4        # TTX_SUBCHUNKS
T4_SLICE = 8192      # kT4Slice
T4_STAGE = 1536      # kT4Stage

# the text of the Shape3 members the derived flags below restate
EXPR = {
    "LPG": "16 / Q0",
    "SUB_": "R1_ <= 32 && Q2_ <= 8",
    "COOP": "(Q1_ * R2_ / NP_ / 16) % kWaves == 0",
    "SUB": "SUB_ && COOP",
    "K0P": "R1 < 32 ? 32 : R1",
    "N1": "Q1 * R2",
    "LDBF": "(N1 + 29) / 32 * 32 + 2",
    "BFS": "TTX_BFS && NP_ > 1 && K0P * LDBF <= 4352",
    "B1ONCE": "NP_ == 1 || BFS",
}

# `using NAME = Shape3<R1, Q1, R2, Q2, NP = 1, MC = 32, Q0 = 4>` as written in the source (macros by name)
TEMPLATES = {
    "S_32_4_32_4": (32, 4, 32, 4, "TTX_NP32", "TTX_MC32"),
    "S_16_4_16_4": (16, 4, 16, 4),
    "S_32_4_32_8": (32, 4, 32, 8, 2, 16),
    "S_16_4_16_8": (16, 4, 16, 8),
    "S_64_4_64_8": (64, 4, 64, 8, 4, 16),
    "S_64_4_64_4": (64, 4, 64, 4, 4, 16),
    "S2_32_4_32_4": (32, 4, 32, 4, 2, 32, 2),
    "S2_16_4_16_4": (16, 4, 16, 4, 1, 32, 2),
    "S2_64_4_64_4": (64, 4, 64, 4, 4, 32, 2),
    "S_32_8_32_8": (32, 8, 32, 8, 4, 16),
    "S2_32_2_32_4": (32, 2, 32, 4, 1, 32, 2),
    "S2_64_2_64_4": (64, 2, 64, 4, 2, 32, 2),
    "S2_16_2_16_4": (16, 2, 16, 4, 1, 32, 2),
    "S_16_8_16_8": (16, 8, 16, 8, 4, 16),
    "S_64_8_64_8": (64, 8, 64, 8, 8, 16),
    "S_32_8_32_16": (32, 8, 32, 16, 4, 16),
    "S_16_8_16_16": (16, 8, 16, 16, 4, 16),
    "S_64_8_64_16": (64, 8, 64, 16, 8, 16),
    "S_32_16_32_16": (32, 16, 32, 16, 8, 16),
    "S_16_16_16_16": (16, 16, 16, 16, 8, 16),
    "S_64_16_64_16": (64, 16, 64, 16, 16, 16),
    "S_32_4_32_32": (32, 4, 32, 32, 2, 16),
    "S_16_4_16_32": (16, 4, 16, 32, 1, 16),
    "S_32_8_32_32": (32, 8, 32, 32, 4, 16),
    "S_16_8_16_32": (16, 8, 16, 32, 4, 16),
    "S_32_16_32_32": (32, 16, 32, 32, 8, 16),
    "S_16_16_16_32": (16, 16, 16, 32, 8, 16),
    "S_128_4_128_4": (128, 4, 128, 4, 4, 16),
    "S_128_4_128_8": (128, 4, 128, 8, 4, 16),
    "S_128_8_128_8": (128, 8, 128, 8, 8, 16),
}

# spec_match's cands[]: (Q0, Q1, Q2, templates for R = 16, 32, 64, 128), in the source's order (the first that holds the geometry)
CANDS = [
    (2, 2, 4, ("S2_16_2_16_4", "S2_32_2_32_4", "S2_64_2_64_4", None)),
    (2, 4, 4, ("S2_16_4_16_4", "S2_32_4_32_4", "S2_64_4_64_4", None)),
    (4, 4, 4, ("S_16_4_16_4", "S_32_4_32_4", "S_64_4_64_4", "S_128_4_128_4")),
    (4, 4, 8, ("S_16_4_16_8", "S_32_4_32_8", "S_64_4_64_8", "S_128_4_128_8")),
    (4, 8, 8, ("S_16_8_16_8", "S_32_8_32_8", "S_64_8_64_8", "S_128_8_128_8")),
    (4, 8, 16, ("S_16_8_16_16", "S_32_8_32_16", "S_64_8_64_16", None)),
    (4, 4, 32, ("S_16_4_16_32", "S_32_4_32_32", None, None)),
    (4, 16, 16, ("S_16_16_16_16", "S_32_16_32_16", "S_64_16_64_16", None)),
    (4, 8, 32, ("S_16_8_16_32", "S_32_8_32_32", None, None)),
    (4, 16, 32, ("S_16_16_16_32", "S_32_16_32_32", None, None)),
]
MATCH_LIMITS = dict(q0=4, q1=16, q2=32, r=128)  # spec_match: beyond, no template


class Shape:
    """the members of Shape3<...> the walk depends on"""

    def __init__(self, name):
        a = [{"TTX_NP32": TTX_NP32, "TTX_MC32": TTX_MC32}.get(x, x) for x in TEMPLATES[name]]
        a = a + [1, 32, 4][len(a) - 4:]
        self.name = name
        self.R1, self.Q1, self.R2, self.Q2, self.NP, self.MC, self.Q0 = a
        self.LPG = 16 // self.Q0
        self.SUB_ = self.R1 <= 32 and self.Q2 <= 8
        self.COOP = (self.Q1 * self.R2 // self.NP // 16) % K_WAVES == 0
        self.SUB = self.SUB_ and self.COOP
        self.K0P = 32 if self.R1 < 32 else self.R1
        self.N1 = self.Q1 * self.R2
        self.LDBF = (self.N1 + 29) // 32 * 32 + 2
        self.BFS = bool(TTX_BFS) and self.NP > 1 and self.K0P * self.LDBF <= 4352
        self.B1ONCE = self.NP == 1 or self.BFS
        self.D = self.Q0 * self.Q1 * self.Q2


SHAPES = {name: Shape(name) for name in TEMPLATES}


def spec_match(q, ranks, exact_only=False):
    """-> (template name or None, pad).  q: three factors; ranks: [r1, r2].  exact_only: ttx_debug_skip bit 15"""
    if len(q) != 3:
        return None, False
    q0, q1, q2 = (int(x) for x in q)
    r1, r2 = (int(x) for x in ranks)
    L = MATCH_LIMITS
    if q0 > L["q0"] or q1 > L["q1"] or q2 > L["q2"] or r1 > L["r"] or r2 > L["r"]:
        return None, False
    rmax = max(r1, r2)
    R = 16 if rmax <= 16 else (32 if rmax <= 32 else (64 if rmax <= 64 else 128))
    ri = {16: 0, 32: 1, 64: 2, 128: 3}[R]
    for Q0, Q1, Q2, ids in CANDS:
        if q0 > Q0 or q1 > Q1 or q2 > Q2 or ids[ri] is None:
            continue
        if (q0, q1, q2, r1, r2) == (Q0, Q1, Q2, R, R):
            return ids[ri], False
        if exact_only:
            return None, False
        real = q0 * r1 * q1 * r2 + q0 * q1 * r2 * q2
        padded = Q0 * R * Q1 * R + Q0 * Q1 * R * Q2
        if real * MAX_PAD_WASTE < padded:
            return None, False
        return ids[ri], True
    return None, False


def t4_merged(q, ranks):
    """four cores on the three-core kernels (t4_merge_dims): -> (q of the three-core geometry, its [r1, r2]) or None.
    q: four factors; ranks: [r1, r2, r3]"""
    if len(q) != 4:
        return None
    q0, q1, q2, q3 = (int(x) for x in q)
    r1, r2, r3 = (int(x) for x in ranks)
    if q2 * q3 > 32 or q3 > 8 or r2 * q2 * r3 > T4_SLICE or r3 > 128 or r2 * q2 * q3 + r3 * q3 > T4_STAGE:
        return None
    q3d, r3d = [q0, q1, q2 * q3], [r1, r2]
    return (q3d, r3d) if spec_match(q3d, r3d)[0] else None


def match_any(q, ranks):
    """spec_match of a three-core geometry, or of what a four-core one merges onto -> (template or None, pad)"""
    if len(q) == 4:
        m = t4_merged(q, ranks)
        return spec_match(*m) if m else (None, False)
    return spec_match(q, ranks)


def spec_mc(q, ranks, nnz, knob64=False):
    """lookups per plan chunk (spec_mc): Shape3::MC, times SUBCHUNKS for a SUB template at a large batch or under the knob"""
    name, _ = match_any(q, ranks)
    if name is None:
        return 0
    s = SHAPES[name]
    return s.MC * (SUBCHUNKS if (s.SUB and (nnz >= SUBCHUNK_NNZ or knob64)) else 1)


def walk_counts(name):
    """the lookup counts of a template's walk cases: two sub-chunks with one lookup in the second; two full ones; three with a
    last group that is not whole; a full chunk; a second chunk of one sub-chunk; three chunks, the last with a partial sub-chunk"""
    s = SHAPES[name]
    M = s.MC
    return [M + 1, 2 * M, 3 * M - 1, 4 * M, 4 * M + 1, 9 * M + s.LPG + 1]


# ---- the case table of tests/test_spec_walk_gpu.py --------------------------------------------------------------------------------
SUB_TEMPLATES = ("S_32_4_32_4", "S2_32_4_32_4", "S_16_4_16_4", "S_32_4_32_8", "S_16_4_16_8", "S2_16_4_16_4", "S2_32_2_32_4", "S_32_8_32_8")
NOT_B1ONCE = ("S_32_8_32_8",)   # the SUB templates whose walk re-stages the core-1 block in every pass of every sub-chunk
P3, P4 = [5, 6, 7], [4, 5, 3, 4]

# template -> (q, [r1, r2])
EXACT = {name: ([SHAPES[name].Q0, SHAPES[name].Q1, SHAPES[name].Q2], [SHAPES[name].R1, SHAPES[name].R2]) for name in SUB_TEMPLATES}
PADDED = {
    "S2_32_2_32_4": ([2, 2, 3], [20, 24]),
    "S2_16_4_16_4": ([2, 3, 4], [12, 16]),
    "S2_32_4_32_4": ([2, 3, 3], [20, 32]),   # D = 18: the scalar paths
    "S_16_4_16_4": ([3, 4, 4], [13, 12]),
    "S_32_4_32_4": ([4, 4, 4], [24, 24]),
    "S_16_4_16_8": ([3, 4, 5], [13, 12]),    # the reference tests' own geometry
    "S_32_4_32_8": ([4, 3, 7], [24, 30]),    # (r2 % 4 != 0)
    "S_32_8_32_8": ([4, 5, 7], [20, 28]),
}
# four cores that merge onto the template, exact: template -> (q, [r1, r2, r3]); p = P4
FOUR_CORES = {
    "S_32_8_32_8": ([4, 8, 4, 2], [32, 32, 8]),
    "S2_32_4_32_4": ([2, 4, 2, 2], [32, 32, 16]),
    "S_32_4_32_4": ([4, 4, 2, 2], [32, 32, 8]),
    "S_16_4_16_4": ([4, 4, 2, 2], [16, 16, 4]),
    "S_32_4_32_8": ([4, 4, 2, 4], [32, 32, 8]),
    "S_16_4_16_8": ([4, 4, 4, 2], [16, 16, 5]),
    "S2_16_4_16_4": ([2, 4, 2, 2], [16, 16, 8]),
    "S2_32_2_32_4": ([2, 2, 2, 2], [32, 32, 4]),
}
# the extra cases (weights, a live count below the length, three tables, every core-1 slice in one launch) run on these
EXTRA_TEMPLATES = ("S_32_8_32_8", "S2_16_4_16_4")
EXTRA_KINDS = ("weights", "live", "three_tables", "all_slices")


def four_core_reachable(name):
    """a four-core geometry can merge onto the template, exact: its last factor splits as q2 q3 with 2 <= q3 <= 8 within
    t4_merge_dims' limits (r3 = 1 is the smallest core-2 slice and staging)"""
    s = SHAPES[name]
    return any(s.Q2 % q3 == 0 and t4_merged([s.Q0, s.Q1, s.Q2 // q3, q3], [s.R1, s.R2, 1]) is not None for q3 in range(2, 9))
