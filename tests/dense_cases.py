"""The cases of the dense member tables' tests (tests/test_dense_tables_gpu.py, tests/test_dense_shapes_gpu.py), and a numpy
mirror of the host-side choices of csrc/ttx_dense.hip that decide which path a case takes.  No torch, no engine: the builders
take the split length C as an argument (the GPU files pass dense_bags_info(...)["split"], tests/test_dense_tables_cpu.py the
value it reads from the source), so that the CPU suite can check what every case reaches (test_dense_tables_cpu.py
`test_new_cases_reach_what_they_are_for`) and pins the mirror to the source text."""
import functools

import numpy as np

import dense_ref as DR

ES = [3, 1, 24, 1460]
PADS = [2, None, 5, 0]
# the 16 Criteo tables below 10,000 rows: the tables MixedTTEmbeddingBag(dense_below=10000) keeps uncompressed in the benchmark
CRITEO_DENSE = [1460, 583, 305, 24, 633, 3, 5683, 3194, 27, 10, 5652, 2173, 4, 18, 15, 105]

# ---- the mirror of csrc/ttx_dense.hip (pinned by tests/test_dense_tables_cpu.py::test_mirror_of_the_host_side_choices) ----
WAVE = 64
SPLIT = 32             # kDenseSplit
CHUNKS_PER_TRIP = 4    # dense_row_grad: j += 4 * kDenseSplit
FLIGHT = 8             # kDenseFlight
THREADS = 256          # kDT
FWD_SLOTS_IN_FLIGHT = 4  # the forward: j += 4 * G
FWD_GRID_BAGS = 4096 * (THREADS // WAVE)  # the forward's grid cap, in bags (one wave per bag)
KEYS_GRID_POSITIONS = 8192 * THREADS      # dense_keys_kernel's grid cap, in positions
MAX_TABLES = 64        # TTX_MAX_TABLES_MIXED


def sort_passes(R):
    """dense_sort_passes: the bytes of the largest key, R"""
    bits = int(R).bit_length()
    return 1 if bits < 8 else (bits + 7) // 8


def lanes_log2(DV):
    """dense_lanes_log2"""
    l = 0
    while (1 << l) < DV and (1 << l) < WAVE:
        l += 1
    return l


def layout(D, aligned=True):
    """-> (W floats per lane, DV column vectors, LPR lanes per row, G row groups per wave): dense_vec4 and dense_lanes_log2"""
    W = 4 if D % 4 == 0 and aligned else 1
    DV = D // W
    LPR = 1 << lanes_log2(DV)
    return W, DV, LPR, WAVE // LPR


def sorted_keys(c):
    """the backward's sorted order from numpy alone: keys as dense_keys_kernel defines them (row + 1; 0 at padding and where no
    bag covers the position), stable descending -> (keys sorted, the positions n in that order)"""
    _, row = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], c["pads"])
    keys = row + 1
    order = np.argsort(-keys, kind="stable")
    return keys[order], order


def runs(c):
    """-> (key, head position in the sorted order, length) of every run of a live key, in sorted order"""
    ks, _ = sorted_keys(c)
    if ks.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    length = np.diff(np.concatenate([head, [ks.size]]))
    keep = ks[head] > 0
    return ks[head][keep], head[keep], length[keep]


# ---------------------------------------------------------------------------------------------------------------- builders
def _split_case(L, D, alone_last=False):
    """tables [3, 24], B = 37: row 0 of table 0 is looked up exactly L times, its lookups spread over the bags between others.
    alone_last: the table's last bag holds exactly one of them -- the run's last lookup in index order is then its bag's only
    lookup of the row, so it wins columns in max mode and the run's last chunk is no sum of zeros in any mode"""
    rs = np.random.RandomState(L)
    B, idx, off = 37, [], [0]
    per = [L // B + (1 if b < L % B else 0) for b in range(B)]
    if alone_last:
        per = [(L - 1) // (B - 1) + (1 if b < (L - 1) % (B - 1) else 0) for b in range(B - 1)] + [1]
    for b in range(B):
        bag = [0] * per[b] + rs.randint(1, 3, size=2).tolist()
        rs.shuffle(bag)
        idx += bag
        off.append(len(idx))
    for b in range(B):
        idx += rs.randint(0, 24, size=int(rs.randint(0, 4))).tolist()
        off.append(len(idx))
    idx = np.asarray(idx, np.int64)
    assert int((idx[:off[B]] == 0).sum()) == L
    return dict(Es=[3, 24], B=B, D=D, idx=idx, off=np.asarray(off, np.int64), pads=None,
                psw=rs.uniform(0.5, 1.5, size=idx.size).astype(np.float32))


def _general(D, B, seed, **kw):
    idx, off, psw = DR.make_batch(seed, ES, B, pad=PADS, **kw)
    return dict(Es=ES, B=B, D=D, idx=idx, off=off, psw=psw, pads=PADS)


def _from_bags(Es, B, D, bags, pads, seed):
    """bags: one list of indices per bag, table-major"""
    assert len(bags) == len(Es) * B
    idx = np.asarray([i for bag in bags for i in bag], np.int64)
    off = np.concatenate([[0], np.cumsum([len(bag) for bag in bags])]).astype(np.int64)
    psw = np.random.RandomState(seed).uniform(0.5, 1.5, size=idx.size).astype(np.float32)
    return dict(Es=list(Es), B=B, D=D, idx=idx, off=off, psw=psw, pads=pads)


def _hot_case(hot, D=64, pads=None, seed=0, Es=(3, 24), B=37):
    """hot = {(table, row): L}: every such row is looked up exactly L times, spread over its table's bags between one or two
    lookups of the table's other rows (cold: a few lookups each); with `pads`, the tables' padding values and the merged batches'
    sentinel -1 are sprinkled in as well"""
    rs = np.random.RandomState(seed)
    bags = []
    for t, E in enumerate(Es):
        mine = {r: L for (tt, r), L in hot.items() if tt == t}
        pad = None if pads is None else pads[t]
        cold = [r for r in range(E) if r not in mine and r != pad]
        for b in range(B):
            bag = []
            for r, L in mine.items():
                bag += [r] * (L // B + (1 if b < L % B else 0))
            if cold:
                bag += rs.choice(cold, size=int(rs.randint(1, 3))).tolist()
            if pads is not None and b % 3 == 0:
                bag += [-1] if pad is None else [pad, -1]
            rs.shuffle(bag)
            bags.append(bag)
    c = _from_bags(Es, B, D, bags, pads, seed + 1)
    c["hot"] = {int(np.cumsum([0] + list(Es))[t] + r) + 1: L for (t, r), L in hot.items()}  # key -> lookups
    return c


def _boundary_case(R, seed):
    """two tables of R rows in all, D = 8, B = 4: the batch looks up the last row (key R), row 0 and rows on both sides of every
    digit boundary below R.  The last row's lookups alternate with padding in index order: the keys R and 0 share every digit
    but R's highest, so a sort of one pass too few leaves them interleaved, the row in several runs."""
    Es = [R - 7, 7]
    want = sorted({r for r in (0, 1, 2, 253, 254, 255, 256, 257, 510, 511, 512, 65533, 65534, 65535, R - 9, R - 8) if 0 <= r < R - 7})
    rs = np.random.RandomState(seed)
    bags = []
    for b in range(4):
        bag = [int(r) for r in rs.choice(want, size=min(5, len(want)), replace=False)] + [0]
        if b == 2:
            bag += want  # (every one of them at least once)
        bags.append(bag)
    for b in range(4):
        bags.append([6, -1, 6, -1, int(rs.randint(0, 6)), 6, -1][:7 - b])
    return _from_bags(Es, 4, 8, bags, None, seed)


def _three_pass_case():
    """two tables of 70,000 rows: keys of three bytes.  Rows 5 and 65,541 of a table (and 6 / 65,542, 300 / 65,836) differ in
    bits 16 and up only, and their lookups alternate in index order"""
    bags = []
    for t in range(2):
        bags += [[5, 65541, 5, 65541, 5], [65542, 6, 65542, 0, 69999], [300, 65836, 300, -1, 65836, 5], [69999, 65541, 131077 % 70000]]
    return _from_bags([70000, 70000], 4, 8, bags, None, 3)


def _tables_case(T, seed):
    """T tables of cardinalities cycling through 1..7 (the last of more than one row), B = 3; every third table and the last have
    a padding value, which the batch holds; every table receives live lookups"""
    Es = [1 + (t + 1) % 7 for t in range(T)]
    pads = [(E - 1 if t % 2 else 0) if (t % 3 == 2 or t == T - 1) and E > 1 else None for t, E in enumerate(Es)]
    rs = np.random.RandomState(seed)
    bags = []
    for t, E in enumerate(Es):
        live = [r for r in range(E) if r != pads[t]]
        for b in range(3):
            bag = rs.randint(0, E, size=int(rs.randint(0, 4))).tolist()
            if b == 1:
                bag += [live[int(rs.randint(len(live)))]] + ([] if pads[t] is None else [pads[t]])
                rs.shuffle(bag)
            bags.append(bag)
    return _from_bags(Es, 3, 64, bags, pads, seed)


def _stride_case(Es, B, D, lo, hi, seed):
    """bags of lo..hi slots each, drawn uniformly from their table"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(lo, hi + 1, size=len(Es) * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    E = np.repeat(np.asarray(Es, np.int64), B)
    idx = (rs.random_sample(int(off[-1])) * np.repeat(E, lens)).astype(np.int64)
    return dict(Es=list(Es), B=B, D=D, idx=idx, off=off, pads=None, psw=rs.uniform(0.5, 1.5, size=idx.size).astype(np.float32))


KEYS_NNZ = (1 << 21) + 300
KEYS_SMALL = 120000  # lookups of the 3-row table: 40,000 per row, 1,250 chunks


def _keys_case():
    """nnz = 2^21 + 300 over tables of 3 and 100,000 rows, B = 512, D = 4.  The 3-row table takes KEYS_SMALL of the lookups -- runs
    of more than a thousand chunks, and short enough for the plain fp32 sum in index order to stay a useful yardstick --, the
    large table the rest (about 20 lookups of a row)"""
    rs = np.random.RandomState(21)
    B = 512

    def lens(total):
        cut = np.sort(rs.randint(0, total + 1, size=B - 1))
        return np.diff(np.concatenate([[0], cut, [total]]))

    ls = np.concatenate([lens(KEYS_SMALL), lens(KEYS_NNZ - KEYS_SMALL)])
    off = np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)
    idx = np.concatenate([rs.randint(0, 3, size=KEYS_SMALL), rs.randint(0, 100000, size=KEYS_NNZ - KEYS_SMALL)]).astype(np.int64)
    return dict(Es=[3, 100000], B=B, D=4, idx=idx, off=off, pads=None, psw=rs.uniform(0.5, 1.5, size=idx.size).astype(np.float32),
                modes=("sum",), legs=("forward", "dense", "sgd"))


def _offsets_case(last, seed):
    """offsets that do not tile indices: offsets[0] = 3 (three leading positions no bag covers) and offsets[-1] = last(nnz)"""
    c = _general(64, 5, seed, tie_table=2)
    nnz = c["idx"].size
    end = last(nnz)
    off = np.minimum(np.maximum(c["off"], 3), min(end, nnz))
    off[-1] = end
    return dict(c, off=off)


WIDTHS = [1, 2, 4, 8, 65, 100, 256, 512]
LADDER = ["3_0", "4_-1", "4_0", "4_1", "5_0", "8_0", "8_1", "40_7"]  # k_m: a row with exactly k * C + m lookups


@functools.lru_cache(maxsize=None)
def case(name, C):
    if name == "split_scalar":
        c = _split_case(C + 1, 6)
    elif name.startswith("split"):  # split_<k>_<m>: a row with exactly k * C + m lookups
        _, k, more = name.split("_")
        c = _split_case(int(k) * C + int(more), 64)
    elif name == "d64":  # the 16-byte path; a bag of 70 slots (more than the rows in flight); table 2 receives no lookup
        c = _general(64, 37, 1, tie_table=3, silent_table=2, long_bag=(3, 5, 70))
    elif name == "d64_b1":
        c = _general(64, 1, 2, tie_table=3, empty=0)
    elif name == "d64_misaligned":  # a weight view one float off a 16-byte boundary: the scalar path at D = 64
        c = dict(_general(64, 5, 3, tie_table=2), misaligned=True)
    elif name == "d6":
        c = _general(6, 37, 4, tie_table=2, long_bag=(2, 7, 70))
    elif name == "d3_b1":
        c = _general(3, 1, 5, tie_table=3, empty=0)
    elif name == "d260":  # rows wider than 256 floats: the column-block walk
        c = _general(260, 5, 6, tie_table=2, long_bag=(3, 2, 70))
    elif name == "nnz0":
        c = dict(Es=ES, B=4, D=64, idx=np.zeros(0, np.int64), off=np.zeros(17, np.int64), psw=np.zeros(0, np.float32), pads=PADS)
    elif name == "all_padding":  # the tables' padding values and the merged batches' sentinel, nothing else
        B = 4
        idx = np.concatenate([np.full(2 * B, 2), np.full(2 * B, -1), np.full(2 * B, 5), np.full(2 * B, 0)]).astype(np.int64)
        c = dict(Es=ES, B=B, D=64, idx=idx, off=np.arange(0, 8 * B + 1, 2, dtype=np.int64), pads=PADS,
                 psw=np.ones(idx.size, np.float32))
    # ---- the cases of tests/test_dense_shapes_gpu.py
    elif name.startswith("ladder6_"):  # the scalar layout of the same
        _, k, more = name.split("_")
        c = _split_case(int(k) * C + int(more), 6, alone_last=True)
    elif name.startswith("ladder_"):
        _, k, more = name.split("_")
        c = _split_case(int(k) * C + int(more), 64, alone_last=True)
    elif name == "place_first":  # the last row of the last table: the largest key, its run at sorted position 0
        c = _hot_case({(1, 23): 4 * C + 1}, seed=11)
    elif name == "place_middle":
        c = _hot_case({(1, 10): 4 * C + 1}, seed=12)
    elif name == "place_row0_padded":  # row 0 behind every other run, the key-0 tail of padding behind it
        c = _hot_case({(0, 0): 4 * C + 1}, pads=[2, 7], seed=13)
    elif name == "place_two":  # runs back to back, lengths in sorted order
        c = _hot_case({(1, 12): 4 * C + 1, (1, 11): 2 * C}, seed=14)
    elif name == "place_three":
        c = _hot_case({(1, 12): 4 * C + 1, (1, 11): 2 * C, (1, 10): C + 1}, seed=15)
    elif name.startswith("rows_"):  # rows_<R>: the digit boundaries of the sort's pass count
        c = _boundary_case(int(name.split("_")[1]), 31)
    elif name == "three_pass":
        c = _three_pass_case()
    elif name.startswith("tables_"):
        c = _tables_case(int(name.split("_")[1]), 41)
    elif name == "fwd_stride_d4":  # 16,448 bags: past the forward's grid cap, at the narrowest 16-byte layout
        c = _stride_case([1 + (t + 1) % 7 for t in range(64)], 257, 4, 0, 2, 51)
    elif name == "fwd_stride_workload":  # the benchmark's 32,768 bags, one or two slots each
        c = _stride_case(CRITEO_DENSE, 2048, 64, 1, 2, 52)
    elif name == "keys_stride":
        c = _keys_case()
    elif name.startswith("width_"):  # a bag of 300 slots: a second trip of the forward's slot loop at every lane layout
        c = _general(int(name.split("_")[1]), 5, 61, tie_table=2, long_bag=(3, 2, 300))
    elif name == "misaligned_d_out":  # grad_output one float off a 16-byte boundary: a 16-byte forward, a scalar backward
        c = dict(_general(64, 5, 71, tie_table=2), misaligned_d_out=True)
    elif name == "misaligned_state":  # the same for the element-wise Adagrad state (the other legs stay on the 16-byte route)
        c = dict(_general(64, 5, 72, tie_table=2), misaligned_state=True)
    elif name == "offsets_short":  # three leading and four trailing positions that no bag covers
        c = _offsets_case(lambda nnz: nnz - 4, 81)
    elif name == "offsets_beyond":  # a closing entry beyond nnz: clamped
        c = _offsets_case(lambda nnz: nnz + 5, 82)
    else:
        raise KeyError(name)
    c = dict(c)
    c["base"] = np.concatenate([[0], np.cumsum(c["Es"])]).astype(np.int64)
    R = int(c["base"][-1])
    rs = np.random.RandomState(77)
    c["w"] = rs.uniform(-1, 1, size=(R, c["D"])).astype(np.float32)
    c["d_out"] = rs.standard_normal((len(c["off"]) - 1, c["D"])).astype(np.float32)
    # a live, all-distinct Adagrad state
    c["s_elem"] = (0.5 + 1e-4 * np.arange(R * c["D"])).reshape(R, c["D"]).astype(np.float32)
    c["s_row"] = (0.5 + 1e-3 * np.arange(R)).astype(np.float32)
    assert np.unique(c["s_elem"]).size == c["s_elem"].size and np.unique(c["s_row"]).size == R
    return c


OLD_CASES = ["d64", "d64_b1", "d64_misaligned", "d6", "d3_b1", "d260", "split_1_0", "split_1_1", "split_2_0", "split_2_1",
             "split_scalar", "nnz0", "all_padding"]
PLACEMENT = ["place_first", "place_middle", "place_row0_padded", "place_two", "place_three"]
BOUNDARIES = ["rows_255", "rows_256", "rows_65535", "rows_65536", "three_pass"]
TABLES = ["tables_5", "tables_33", "tables_64"]
NEW_CASES = ([f"ladder_{k}" for k in LADDER] + ["ladder6_4_1"] + PLACEMENT + BOUNDARIES + TABLES
             + ["fwd_stride_d4", "fwd_stride_workload"] + [f"width_{d}" for d in WIDTHS]
             + ["misaligned_d_out", "misaligned_state", "offsets_short", "offsets_beyond"])
LARGE_CASES = ["keys_stride"]  # (its own test: sum only, three legs)
