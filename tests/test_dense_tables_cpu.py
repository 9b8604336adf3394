"""CPU tests (no GPU) of the dense member tables: the float64 restatement tests/dense_ref.py against torch's own F.embedding_bag,
autograd and optimizers; the argument checks of the C ABI (every error before anything touches a device); the selection helper
of MixedTTEmbeddingBag(dense_below=, dense=); and the compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_cases as DC
import dense_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = [3, 1, 24, 1460]
B_, D_ = 7, 6
PADS = [2, None, 5, 0]
BASE = np.concatenate([[0], np.cumsum(ES)]).astype(np.int64)


def weights(seed=0):
    return np.random.RandomState(seed).uniform(-1, 1, size=(int(BASE[-1]), D_))


def torch_tables(w, indices, offsets, mode, pads, psw):
    """one F.embedding_bag per table on float64 leaves -> (leaves, out [tables * B, D])"""
    leaves, outs = [], []
    for t in range(len(ES)):
        leaf = torch.tensor(w[BASE[t]:BASE[t + 1]], dtype=torch.float64, requires_grad=True)
        s, e = int(offsets[t * B_]), int(offsets[(t + 1) * B_])
        off = torch.from_numpy(offsets[t * B_:(t + 1) * B_ + 1] - s)
        pw = None if psw is None else torch.from_numpy(psw[s:e].astype(np.float64))
        outs.append(F.embedding_bag(torch.from_numpy(indices[s:e]), leaf, off, mode=mode, per_sample_weights=pw,
                                    include_last_offset=True, padding_idx=None if pads is None else pads[t]))
        leaves.append(leaf)
    return leaves, torch.cat(outs)


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_reference_forward_and_gradient_equal_torch(mode, padded):
    pads = PADS if padded else None
    idx, off, psw = DR.make_batch(3, ES, B_, pad=pads, tie_table=2)
    psw = psw if mode == "sum" else None
    w = weights()
    if mode == "max":  # a tie inside a bag: the bag's first two slots hold the same row
        s = int(off[2 * B_])
        assert idx[s] == idx[s + 1]
    lens = np.diff(off)
    assert (lens == 0).sum() >= len(lens) // 5, "a fifth of the bags are empty"
    out, live, arg = DR.forward(w, idx, off, BASE, B_, mode, pads, psw)
    leaves, t_out = torch_tables(w, idx, off, mode, pads, psw)
    np.testing.assert_allclose(out, t_out.detach().numpy(), rtol=1e-12, atol=1e-14)
    if padded:
        assert live[1] == 0 and not out[1].any(), "a bag of padding only is zero"
    d_out = np.random.RandomState(5).standard_normal(out.shape)
    t_out.backward(torch.from_numpy(d_out))
    G, touched, _ = DR.row_grads(w, idx, off, BASE, B_, d_out, mode, pads, psw)
    for t in range(len(ES)):
        np.testing.assert_allclose(G[BASE[t]:BASE[t + 1]], leaves[t].grad.numpy(), rtol=1e-12, atol=1e-14)
    assert not G[~touched].any()
    if mode == "mean" and padded:  # the divisor is the live count, not the bag's length: the case holds such a bag
        assert ((live > 0) & (live < lens)).any()


def test_reference_weight_gradient_equals_torch():
    idx, off, psw = DR.make_batch(4, ES, B_, pad=PADS)
    w = weights(1)
    d_out = np.random.RandomState(6).standard_normal((len(off) - 1, D_))
    pw = torch.tensor(psw.astype(np.float64), requires_grad=True)
    outs = []
    for t in range(len(ES)):
        s, e = int(off[t * B_]), int(off[(t + 1) * B_])
        outs.append(F.embedding_bag(torch.from_numpy(idx[s:e]), torch.from_numpy(w[BASE[t]:BASE[t + 1]]),
                                    torch.from_numpy(off[t * B_:(t + 1) * B_ + 1] - s), mode="sum", per_sample_weights=pw[s:e],
                                    include_last_offset=True, padding_idx=PADS[t]))
    torch.cat(outs).backward(torch.from_numpy(d_out))
    _, _, d_psw = DR.row_grads(w, idx, off, BASE, B_, d_out, "sum", PADS, psw)
    np.testing.assert_allclose(d_psw, pw.grad.numpy(), rtol=1e-12, atol=1e-14)
    bag, row = DR.lookups(idx, off, BASE, B_, PADS)
    assert (row < 0).any() and not d_psw[row < 0].any(), "0 at padding"


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_reference_three_steps_equal_torch_optimizers(opt):
    lr, eps = 0.1, 1e-10
    w = weights(2)
    leaves = [torch.tensor(w[BASE[t]:BASE[t + 1]], dtype=torch.float64, requires_grad=True) for t in range(len(ES))]
    o = torch.optim.SGD(leaves, lr=lr) if opt == "sgd" else torch.optim.Adagrad(leaves, lr=lr, eps=eps)
    state = np.zeros_like(w)
    for step in range(3):
        idx, off, _ = DR.make_batch(10 + step, ES, B_, pad=PADS)
        d_out = np.random.RandomState(20 + step).standard_normal((len(off) - 1, D_))
        G, touched, _ = DR.row_grads(w, idx, off, BASE, B_, d_out, "sum", PADS)
        if opt == "sgd":
            w = DR.sgd(w, G, touched, lr)
        else:
            w, state = DR.adagrad(w, state, G, touched, lr, eps)
        o.zero_grad()
        outs = []
        for t in range(len(ES)):
            s, e = int(off[t * B_]), int(off[(t + 1) * B_])
            outs.append(F.embedding_bag(torch.from_numpy(idx[s:e]), leaves[t], torch.from_numpy(off[t * B_:(t + 1) * B_ + 1] - s),
                                        mode="sum", include_last_offset=True, padding_idx=PADS[t]))
        torch.cat(outs).backward(torch.from_numpy(d_out))
        o.step()
        for t in range(len(ES)):
            np.testing.assert_allclose(w[BASE[t]:BASE[t + 1]], leaves[t].detach().numpy(), rtol=1e-11, atol=1e-13,
                                       err_msg=f"{opt} step {step} table {t}")


def test_reference_rowwise_adagrad_by_hand():
    w, s = np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([0.5, 0.25])
    G, touched = np.array([[3.0, 4.0], [0.0, 0.0]]), np.array([True, False])
    w1, s1 = DR.rowwise_adagrad(w, s, G, touched, 0.1, 1e-3)
    assert s1[0] == 0.5 + 12.5 and s1[1] == 0.25
    np.testing.assert_allclose(w1[0], w[0] - 0.1 * G[0] / (np.sqrt(13.0) + 1e-3), rtol=1e-15)
    assert (w1[1] == w[1]).all()


def test_reference_clamps_bad_indices_into_their_table():
    bag, row = DR.lookups(np.array([5, -7, 99]), np.array([0, 1, 2, 3]), np.array([0, 3, 4, 28]), 1)
    assert row.tolist() == [2, -1, 27]


# ------------------------------------------------------------------------- the mirror of the host-side choices, and the cases
with open(os.path.join(ROOT, "fbtt-embedding_amd", "csrc", "ttx_dense.hip")) as f:
    SRC = f.read()
SQ = re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", re.sub(r"\\\n", "", SRC)))  # (macro continuations joined, comments and spaces out)
UPDATE = "update tests/dense_cases.py (the mirror and the case table of tests/test_dense_shapes_gpu.py)"


def _const(name, text=SRC):
    m = re.findall(rf"constexpr int {name} = (\d+);", text)
    assert len(m) == 1, f"{name}: {len(m)} definitions"
    return int(m[0])


def _has(text, what, count=1):
    assert SQ.count(re.sub(r"\s+", "", text)) == count, f"{what} is no longer `{text}`: {UPDATE}"


C_SRC = _const("kDenseSplit")


def test_mirror_of_the_host_side_choices():
    """tests/dense_cases.py restates the constants and host functions of csrc/ttx_dense.hip that decide which path a batch takes;
    a retuned constant fails here and names the case table to update"""
    with open(os.path.join(ROOT, "fbtt-embedding_amd", "csrc", "ttx_internal.h")) as f:
        assert _const("kWave", f.read()) == DC.WAVE
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        assert re.findall(r"^#define TTX_MAX_TABLES_MIXED (\d+)\b", f.read(), flags=re.M) == [str(DC.MAX_TABLES)]
    assert _const("kDenseSplit") == DC.SPLIT and _const("kDenseFlight") == DC.FLIGHT and _const("kDT") == DC.THREADS, UPDATE
    _has("constexpr int kDW = kDT / kWave;", "waves per work-group")
    _has("constexpr int kDenseBases = TTX_MAX_TABLES_MIXED + 1;", "the staged row bases")
    # dense_row_grad: CHUNKS_PER_TRIP chunk sums per trip
    n = DC.CHUNKS_PER_TRIP
    _has(f"for (long long j = i; j < nnz; j += {n} * kDenseSplit) {{", "dense_row_grad's chunk stride")
    _has(f"float v[{n}][W]; bool more = true; #pragma unroll for (int u = 0; u < {n}; ++u) {{ const long long jj = j + (long long)u * "
         "kDenseSplit;", "dense_row_grad's chunks in flight")
    _has("for (long long j = i; j < end; j += kDenseFlight) {", "dense_list_sum's stride")
    # the forward: FWD_SLOTS_IN_FLIGHT slots of a row group per trip, the grid cap and the stride behind it
    _has(f"for (long long j = s + grp; j < e; j += {DC.FWD_SLOTS_IN_FLIGHT} * G) {{", "the forward's slot stride")
    _has("const int LPR = 1 << lpr_log2, G = kWave >> lpr_log2;", "the forward's lane layout")
    _has("const long long want = (nb + kDW - 1) / kDW; const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);",
         "the forward's grid cap")
    assert DC.FWD_GRID_BAGS == 4096 * (DC.THREADS // DC.WAVE)
    _has("for (long long bag = (long long)blockIdx.x * kDW + threadIdx.x / kWave; bag < nb; bag += (long long)gridDim.x * kDW) {",
         "the forward's grid stride")
    _has("const long long want = (nnz + kDT - 1) / kDT; hipLaunchKernelGGL(dense_keys_kernel, dim3((unsigned)(want < 8192 ? want : "
         "8192)), dim3(kDT),", "the key kernel's grid cap")
    assert DC.KEYS_GRID_POSITIONS == 8192 * DC.THREADS
    _has("for (long long n = (long long)blockIdx.x * kDT + threadIdx.x; n < nnz; n += (long long)gridDim.x * kDT) {",
         "the key kernel's grid stride")
    # the three host functions
    _has("static int dense_sort_passes(int64_t R) { int bits = 0; while (bits < 64 && ((uint64_t)R >> bits)) ++bits; "
         "return bits < 8 ? 1 : (bits + 7) / 8; }", "dense_sort_passes")
    _has("sort_pairs_desc(nnz, keys, vals, sort_ws, &ks, &vs, st, dense_sort_passes(R));", "the sort's pass count")
    _has("const int64_t R = row_base[num_tables];", "the largest key")
    assert [DC.sort_passes(r) for r in (1, 127, 128, 255, 256, 65535, 65536, 140000, (1 << 24) - 1, 1 << 24)] == \
        [1, 1, 1, 1, 2, 2, 3, 3, 3, 4]
    _has("static int dense_lanes_log2(int DV) { int l = 0; while ((1 << l) < DV && (1 << l) < kWave) ++l; return l; }", "dense_lanes_log2")
    assert [DC.lanes_log2(v) for v in (1, 2, 3, 4, 16, 25, 33, 64, 65, 512)] == [0, 1, 2, 2, 4, 5, 6, 6, 6, 6]
    _has("static bool dense_vec4(int32_t D, std::initializer_list<const void*> ptrs) { if (D % 4 != 0) return false; "
         "for (const void* p : ptrs) if (((uintptr_t)p) & 15) return false; return true; }", "dense_vec4")
    _has("const bool v4 = dense_vec4(D, {weight, output, mode == 2 ? (const void*)argmax : nullptr});", "the forward's 16-byte rule")
    _has("const bool v4 = dense_vec4(D, {grad_output, target, part, mode == 2 ? (const void*)argmax : nullptr, "
         "opt == 1 ? (const void*)opt_state : nullptr, d_per_sample_weights ? (const void*)weight : nullptr});",
         "the backward's 16-byte rule (per call: grad_output and the element-wise state decide it too)")
    _has("const int DV = v4 ? D / 4 : D, lg = dense_lanes_log2(DV);", "the lane layout", count=2)
    assert [DC.layout(d) for d in (1, 2, 4, 8, 64, 65, 100, 256, 512)] == \
        [(1, 1, 1, 64), (1, 2, 2, 32), (4, 1, 1, 64), (4, 2, 2, 32), (4, 16, 16, 4), (1, 65, 64, 1), (4, 25, 32, 2), (4, 64, 64, 1),
         (4, 128, 64, 1)]
    assert DC.layout(64, aligned=False) == (1, 64, 64, 1)


SMALL = 20000  # lookups: below, the loop forms of dense_ref are quick enough to be run next to the vectorised ones


@pytest.mark.parametrize("name", DC.OLD_CASES + DC.NEW_CASES)
def test_vectorised_reference_is_the_loop_reference_bit_for_bit(name):
    """every existing case and every new one below 20 k lookups, in the three modes, in float64 and as the fp32 yardstick"""
    c = DC.case(name, C_SRC)
    if c["idx"].size >= SMALL:
        assert name in ("fwd_stride_workload",), f"{name}: {c['idx'].size} lookups"
        return
    a = (c["idx"], c["off"], c["base"], c["B"])
    for x, y in zip(DR.lookups(*a, c["pads"]), DR.lookups_vec(*a, c["pads"])):
        assert np.array_equal(x, y)
    for mode in ("sum", "mean", "max"):
        psw = c["psw"] if mode == "sum" else None
        for dtype in (np.float64, np.float32):
            for loop, vec, more in ((DR.forward, DR.forward_vec, ()), (DR.row_grads, DR.row_grads_vec, (c["d_out"],))):
                want = loop(c["w"], *a, *more, mode, c["pads"], psw, dtype=dtype)
                got = vec(c["w"], *a, *more, mode, c["pads"], psw, dtype=dtype)
                for k, (x, y) in enumerate(zip(want, got)):
                    assert x.dtype == y.dtype and x.shape == y.shape, (mode, dtype, loop.__name__, k)
                    assert np.array_equal(x, y), (mode, dtype, loop.__name__, k, float(np.abs(x - y).max()))


def _window_shared_by_two_chunk_starts(ks, heads, lens, C):
    """aligned windows of C sorted positions that hold the start of a split run's short last chunk AND of the next run's first
    full chunk (dense_slot's two workspace rows per window)"""
    found = []
    for h, L, h2, L2 in zip(heads[:-1], lens[:-1], heads[1:], lens[1:]):
        if L > C and L % C and L2 > C and h + L == h2 and (h + L - L % C) // C == h2 // C:
            found.append(int(h2 // C))
    return found


def test_new_cases_reach_what_they_are_for():
    """every numbered gap of the suite before tests/test_dense_shapes_gpu.py, by a quantity computed from numpy alone: keys as
    dense_keys_kernel defines them, a stable descending sort, the mirror of the host-side choices"""
    C, T = C_SRC, DC.CHUNKS_PER_TRIP
    old = [DC.case(n, C) for n in DC.OLD_CASES]
    old_longest = max(int(DC.runs(c)[2].max()) for c in old if DC.runs(c)[2].size)
    assert old_longest <= T * C, "(what the earlier cases stop at: a run of four chunks)"
    # 1. runs longer than four chunks: the ladder's hot row is row 0 of table 0 (key 1), exactly k C + m lookups long
    trips = {}
    for k in DC.LADDER:
        c = DC.case(f"ladder_{k}", C)
        key, head, length = DC.runs(c)
        L = int(k.split("_")[0]) * C + int(k.split("_")[1])
        assert key[-1] == 1 and length[-1] == L and head[-1] + L == c["idx"].size, "the smallest key: its run ends at nnz"
        trips[k] = -(-(-(-L // C)) // T)  # trips of dense_row_grad's loop over ceil(L / C) chunks
    assert trips == {"3_0": 1, "4_-1": 1, "4_0": 1, "4_1": 2, "5_0": 2, "8_0": 2, "8_1": 3, "40_7": 11}
    c = DC.case("ladder6_4_1", C)
    assert DC.runs(c)[2][-1] == 4 * C + 1 and DC.layout(c["D"])[0] == 1, "the scalar backward over a run of two trips"
    # ... and the run's last chunk counts in every mode: in max mode a lookup adds only the columns it won in its bag, and
    # a bag's later lookups of the same row win none (the first position keeps a tie)
    for name in [f"ladder_{k}" for k in DC.LADDER] + ["ladder6_4_1"]:
        c = DC.case(name, C)
        _, order = DC.sorted_keys(c)
        L = int(DC.runs(c)[2][-1])
        last = order[c["idx"].size - ((L - 1) % C + 1):]  # the positions n of the last chunk's lookups
        bag, _ = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], c["pads"])
        arg = DR.forward_vec(c["w"], c["idx"], c["off"], c["base"], c["B"], "max")[2]
        assert any((arg[bag[n]] == n).any() for n in last), f"{name}: the last chunk's lookups win no column in max mode"
    assert np.log2(DC.runs(DC.case("ladder_40_7", C))[2][-1]) > 10, "the partial kernel's search for a head: more than 10 steps deep"
    # 2. where a split run sits
    def hot_runs(name):
        c = DC.case(name, C)
        key, head, length = DC.runs(c)
        ks, _ = DC.sorted_keys(c)
        at = {int(k): (int(h), int(n)) for k, h, n in zip(key, head, length)}
        for k, L in c["hot"].items():
            assert at[k][1] == L, (name, k)
        return c, ks, key, head, length, [at[k] for k in sorted(c["hot"], reverse=True)]

    c, ks, key, head, length, hot = hot_runs("place_first")
    assert hot == [(0, 4 * C + 1)] and ks[0] == c["base"][-1], "the largest key: a split run at sorted position 0"
    c, ks, key, head, length, hot = hot_runs("place_middle")
    (h, L), = hot
    assert h > 0 and ks[h - 1] > ks[h] and h + L < ks.size and 0 < ks[h + L] < ks[h] and L == 4 * C + 1, "between other runs"
    c, ks, key, head, length, hot = hot_runs("place_row0_padded")
    (h, L), = hot
    assert ks[h] == 1 and L == 4 * C + 1 and h + L < ks.size and not ks[h + L:].any(), "the key-0 tail of padding behind the run"
    assert (c["idx"] == -1).any() and (c["idx"][:c["off"][c["B"]]] == 2).any(), "the sentinel and table 0's padding value"
    for name, want in (("place_two", [4 * C + 1, 2 * C]), ("place_three", [4 * C + 1, 2 * C, C + 1])):
        c, ks, key, head, length, hot = hot_runs(name)
        assert [L for _, L in hot] == want and all(a[0] + a[1] == b[0] for a, b in zip(hot, hot[1:])), "split runs back to back"
        shared = _window_shared_by_two_chunk_starts(ks, head, length, C)
        assert hot[1][0] // C in shared, f"{name}: no window of {C} positions holds a last chunk's and a first chunk's start"
    # 3. the sort's pass count, on both sides of each digit boundary
    passes = {}
    for name in DC.BOUNDARIES:
        c = DC.case(name, C)
        R = int(c["base"][-1])
        key, head, length = DC.runs(c)
        passes[name] = DC.sort_passes(R)
        assert key[0] == R and key[-1] == 1 and c["D"] == 8 and c["B"] <= 8, "the last row (key R) and row 0"
        # one pass fewer sorts by the low digits only: the case must hold keys that then fall into one another's runs
        if passes[name] > 1:
            _, row = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], c["pads"])
            k = row + 1
            kl = k & ((1 << (8 * (passes[name] - 1))) - 1)
            o = np.argsort(-kl, kind="stable")
            n_runs = int((np.diff(k[o]) != 0).sum()) + 1
            assert n_runs > np.unique(k).size, f"{name}: a sort of {passes[name] - 1} pass(es) would still leave every row one run"
    assert passes == {"rows_255": 1, "rows_256": 2, "rows_65535": 2, "rows_65536": 3, "three_pass": 3}
    assert {DC.sort_passes(int(c["base"][-1])) for c in old} <= {1, 2}
    c = DC.case("three_pass", C)
    assert c["Es"] == [70000, 70000] and {6, 65542, 70006, 135542} <= set(DC.runs(c)[0].tolist()), "keys that differ in bits 16 and up"
    # 4. more than four tables
    for name in DC.TABLES:
        c = DC.case(name, C)
        nt = len(c["Es"])
        assert nt == int(name.split("_")[1]) and c["B"] == 3 and set(c["Es"]) <= set(range(1, 8)) and c["pads"][-1] is not None
        _, row = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], c["pads"])
        tab = np.searchsorted(c["base"], row[row >= 0], side="right") - 1
        assert set(tab.tolist()) == set(range(nt)), "every table receives live lookups"
        held = [t for t in range(nt) if c["pads"][t] is not None and
                (c["idx"][c["off"][3 * t]:c["off"][3 * t + 3]] == c["pads"][t]).any()]
        assert len(held) >= min(3, nt // 3) and nt - 1 in held, "padding values on several tables, the last included"
    assert len(DC.case("tables_64", C)["Es"]) == DC.MAX_TABLES and max(len(c["Es"]) for c in old) == 4
    # 5. the grid-stride loops
    for name, nb in (("fwd_stride_d4", 64 * 257), ("fwd_stride_workload", 16 * 2048)):
        c = DC.case(name, C)
        assert len(c["off"]) - 1 == nb > DC.FWD_GRID_BAGS, "a wave of the forward takes more than one bag"
    lens = np.diff(DC.case("fwd_stride_d4", C)["off"])
    assert lens.min() == 0 and lens.max() == 2 and np.diff(DC.case("fwd_stride_workload", C)["off"]).min() == 1
    assert max(len(c["off"]) - 1 for c in old) <= DC.FWD_GRID_BAGS and max(c["idx"].size for c in old) <= DC.KEYS_GRID_POSITIONS
    assert DC.KEYS_NNZ == (1 << 21) + 300 > DC.KEYS_GRID_POSITIONS and DC.KEYS_SMALL // 3 > 1000 * C
    # 6. lane layouts: lanes per row, row groups per wave, slots per trip of the forward's loop against the 300-slot bag
    seen = {}
    for D in DC.WIDTHS:
        c = DC.case(f"width_{D}", C)
        W, DV, LPR, G = DC.layout(D)
        seen[D] = (W, LPR, G, -(-DV // LPR))
        assert c["B"] == 5 and np.diff(c["off"]).max() == 300 > DC.FWD_SLOTS_IN_FLIGHT * G, "a second trip of the slot loop"
        s = int(c["off"][2 * 5])
        assert c["idx"][s] == c["idx"][s + 1], "the tie table: a bag's first two slots hold the same row"
    assert seen == {1: (1, 1, 64, 1), 2: (1, 2, 32, 1), 4: (4, 1, 64, 1), 8: (4, 2, 32, 1), 65: (1, 64, 1, 2), 100: (4, 32, 2, 1),
                    256: (4, 64, 1, 1), 512: (4, 64, 1, 2)}, "(W, lanes per row, row groups, column blocks)"
    assert not {DC.layout(c["D"], not c.get("misaligned"))[:3] for c in old} & {seen[d][:3] for d in (1, 4, 8, 100)}
    # 7. a 16-byte forward with a scalar backward is a flag of the case; the GPU test asserts the pointers' alignment
    assert DC.case("misaligned_d_out", C)["D"] == 64 and DC.case("misaligned_state", C)["D"] == 64
    # 8. offsets that do not tile indices
    for name, last in (("offsets_short", -4), ("offsets_beyond", 5)):
        c = DC.case(name, C)
        nnz = c["idx"].size
        bag, row = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], c["pads"])
        assert c["off"][0] == 3 and c["off"][-1] == nnz + last and (bag[:3] == -1).all() and (bag[3:nnz + min(last, 0)] >= 0).all()
        assert (bag[nnz + min(last, 0):] == -1).all() and ((bag >= 0) & (row < 0)).any(), "uncovered positions, and padding"
        assert (c["idx"][bag < 0] >= 0).any(), "an uncovered position holds a live index: it must contribute nothing"
    assert all(c["off"][0] == 0 and c["off"][-1] == c["idx"].size for c in old)


@pytest.mark.parametrize("name", DC.NEW_CASES + DC.LARGE_CASES)
def test_yardstick_of_every_new_case_stays_under_the_cap(name):
    """The widening rule (twice the plain-fp32 index-order sum's distance from float64) is capped at 5 default bounds; the cap is a
    condition on the case, not a measurement: a case whose yardstick needs more is reshaped (fewer lookups of a row)."""
    import tt_ref64 as R64

    c = DC.case(name, C_SRC)
    for mode in c.get("modes", ("sum", "mean", "max")):
        psw = c["psw"] if mode == "sum" else None
        a = (c["w"], c["idx"], c["off"], c["base"], c["B"])
        out = DR.forward_vec(*a, mode, c["pads"], psw)[0]
        out32 = DR.forward_vec(*a, mode, c["pads"], psw, dtype=np.float32)[0]
        G, _, dp = DR.row_grads_vec(*a, c["d_out"], mode, c["pads"], psw)
        G32, _, dp32 = DR.row_grads_vec(*a, c["d_out"], mode, c["pads"], psw, dtype=np.float32)
        for what, x32, x in (("forward", out32, out), ("G", G32, G), ("d_psw", dp32, dp)):
            u = R64.default_units(x32, x)
            print(f"[dense-tables] {name} {mode} {what}: plain fp32 {u:.3f} default bounds from float64")
            assert 2.0 * u <= R64.WIDEN_CAP, (name, mode, what, u)


# ----------------------------------------------------------------------------------------------------------------- the ABI
i64, i32, vp, f32, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t


def _libs():
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        lib.ttx_dense_bags_forward.argtypes = [i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        lib.ttx_dense_bags_backward_workspace_bytes.restype = sz
        lib.ttx_dense_bags_backward_workspace_bytes.argtypes = [i64, i64, i32]
        lib.ttx_dense_bags_backward.argtypes = [i32, i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, f32, i32, vp, vp,
                                                vp, vp, vp, sz, vp]
        lib.ttx_dense_bags_info.argtypes = [i32, i64, ctypes.POINTER(i32)]
        yield lib


def test_entry_points_are_declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    for name in ("ttx_dense_bags_forward", "ttx_dense_bags_backward", "ttx_dense_bags_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/ttx.h"
    assert re.search(r"\bsize_t\s+ttx_dense_bags_backward_workspace_bytes\s*\(", hdr)


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced; this machine has no GPU: a call that reached the runtime would return -4)"""
    fake, odd = 4096, 4098
    base = (i64 * 3)(0, 3, 27)
    pad = (i64 * 2)(-1, 4)
    for lib in _libs():
        def fwd(**kw):
            a = dict(nt=2, B=4, D=8, nnz=16, idx=fake, off=fake, base=base, pad=None, psw=None, mode=0, w=fake, out=fake,
                     live=None, arg=None)
            a.update(kw)
            return lib.ttx_dense_bags_forward(a["nt"], a["B"], a["D"], a["nnz"], a["idx"], a["off"], a["base"], a["pad"], a["psw"],
                                              a["mode"], a["w"], a["out"], a["live"], a["arg"], None)

        def bwd(**kw):
            a = dict(optim=0, nt=2, B=4, D=8, nnz=16, idx=fake, off=fake, base=base, pad=None, psw=None, mode=0, live=None,
                     arg=None, g=fake, width=0, state=None, w=fake, dw=None, dpsw=None, ws=fake, wsb=1 << 30)
            a.update(kw)
            return lib.ttx_dense_bags_backward(a["optim"], a["nt"], a["B"], a["D"], a["nnz"], a["idx"], a["off"], a["base"],
                                               a["pad"], a["psw"], a["mode"], a["live"], a["arg"], a["g"], 0.1, 1e-8, a["width"],
                                               a["state"], a["w"], a["dw"], a["dpsw"], a["ws"], a["wsb"], None)

        shared = [dict(B=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(B=1 << 30), dict(nt=0), dict(nt=65), dict(base=None),
                  dict(base=(i64 * 3)(1, 3, 27)), dict(base=(i64 * 3)(0, 3, 3)), dict(base=(i64 * 3)(0, 5, 4)), dict(D=0), dict(D=-8),
                  dict(psw=fake, mode=1), dict(psw=fake, mode=2), dict(mode=3), dict(mode=1), dict(mode=2), dict(idx=None),
                  dict(off=None), dict(idx=odd), dict(off=odd), dict(psw=odd), dict(w=None), dict(w=odd)]
        for kw in shared + [dict(out=None), dict(out=odd), dict(mode=1, live=odd), dict(mode=2, arg=odd)]:
            assert fwd(**kw) == -1, ("forward", kw)
            assert b"dense_bags_forward" in lib.ttx_last_error(), lib.ttx_last_error()
        more = [dict(optim=3), dict(optim=-1), dict(width=1), dict(width=8), dict(optim=1, width=0, state=fake),
                dict(optim=1, width=4, state=fake), dict(optim=1, width=8, state=None), dict(optim=1, width=1, state=odd),
                dict(optim=2, width=1, dw=fake), dict(optim=2, dw=None), dict(optim=2, dw=odd), dict(g=None), dict(g=odd),
                dict(mode=1, live=odd), dict(mode=2, arg=odd), dict(dpsw=odd), dict(dpsw=fake, mode=1, live=fake),
                dict(dpsw=fake, optim=2, dw=fake, w=None)]
        for kw in shared + more:
            if kw in (dict(w=None), dict(w=odd)):
                kw = dict(kw, optim=0)
            assert bwd(**kw) == -1, ("backward", kw)
            assert b"dense_bags_backward" in lib.ttx_last_error(), lib.ttx_last_error()
        need = lib.ttx_dense_bags_backward_workspace_bytes(8, 16, 8)
        assert need > 0
        for kw in (dict(wsb=need - 1), dict(ws=None), dict(wsb=0)):
            assert bwd(**kw) == -2, ("workspace", kw)  # TTX_EWORKSPACE
            assert b"workspace" in lib.ttx_last_error()
        # a padding array is read, not refused; per-table padding given misaligned is
        assert fwd(pad=ctypes.cast(ctypes.addressof(pad) + 4, vp)) == -1
        out = (i32 * 2)()
        assert lib.ttx_dense_bags_info(64, 1000, out) == 0 and out[0] > 0 and out[1] >= 0
        assert lib.ttx_dense_bags_info(0, 1000, out) == -1 and lib.ttx_dense_bags_info(64, 10, None) == -1


def test_engine_exposes_the_dense_calls():
    import tt_embeddings as E

    assert callable(E.dense_bags_forward) and callable(E.dense_bags_backward)
    info = E.dense_bags_info(64, 1000)
    assert info["split"] > 0 and set(info) == {"split", "one_launch"}
    with pytest.raises(RuntimeError):  # (no CPU path in the engine)
        E.dense_bags_forward(torch.zeros(4, dtype=torch.int64), torch.arange(5), [0, 3], torch.zeros(3, 8))


def test_module_refuses_cpu_tensors_and_bad_keywords():
    import ttx_dense as TD

    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, mode="min", device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, padding_idx=[1], device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, padding_idx=[3, None], device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3] * 65, 8, device="cpu")
    m = TD.DenseTableBatchedEmbeddingBag(ES, D_, optimizer=TD.OptimType.EXACT_ROWWISE_ADAGRAD, padding_idx=[-1, None, 5, 0], device="cpu")
    assert m.padding_idx == [2, None, 5, 0] and m.row_base == BASE.tolist()
    assert tuple(m.weight.shape) == (int(BASE[-1]), D_) and tuple(m.optimizer_state.shape) == (int(BASE[-1]),)
    assert list(m.state_dict()) == ["weight", "optimizer_state"]
    for k, e in enumerate(ES):
        tw = m.table_weight(k)
        assert tuple(tw.shape) == (e, D_) and float(tw.abs().max()) <= 1.0 / np.sqrt(e)
        assert tw.data_ptr() == m.weight.data_ptr() + int(BASE[k]) * D_ * 4, "a view"
    assert TD.DenseTableBatchedEmbeddingBag(ES, D_, device="cpu").optimizer_state.numel() == 0
    assert tuple(TD.DenseTableBatchedEmbeddingBag(ES, D_, optimizer=TD.OptimType.EXACT_ADAGRAD, device="cpu").optimizer_state.shape) \
        == (int(BASE[-1]), D_)
    with pytest.raises(RuntimeError):
        m(torch.zeros(8, dtype=torch.int64), torch.arange(9))


# ------------------------------------------------------------------------------------------------- the selection helper
def test_selection_helper():
    from ttx_dense import dense_table_flags, dense_table_groups

    Es = [3, 200000, 1460, 24, 50000, 583]
    assert dense_table_flags(Es) == [False] * 6 and dense_table_groups(dense_table_flags(Es)) == []
    assert dense_table_flags(Es, dense_below=10000) == [True, False, True, True, False, True]
    assert dense_table_flags(Es, dense_below=1460) == [True, False, False, True, False, True], "strictly below"
    assert dense_table_flags(Es, 10000, dense=[False, True, False, False, False, False]) == [False, True] + [False] * 4, \
        "`dense` overrides dense_below"
    assert dense_table_groups([True, False, True, True, False, True]) == [[0, 2, 3, 5]]
    with pytest.raises(ValueError):
        dense_table_flags(Es, dense=[True])
    with pytest.raises(ValueError):
        dense_table_flags(Es, dense_below=-1)
    many = dense_table_groups([True] * 70 + [False] + [True] * 60)
    assert [len(g) for g in many] == [64, 64, 2] and many[1][:7] == [64, 65, 66, 67, 68, 69, 71] and many[2] == [129, 130]
    criteo = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10, 5652, 2173,
              4, 7046547, 18, 15, 286181, 105, 142572]
    assert sum(dense_table_flags(criteo, 10000)) == 16 and sum(dense_table_flags(criteo, 10 ** 6)) == 21


def test_mixed_module_accepts_the_keywords():
    import inspect

    import ttx_mixed

    sig = inspect.signature(ttx_mixed.MixedTTEmbeddingBag.__init__)
    assert sig.parameters["dense_below"].default == 0 and sig.parameters["dense"].default is None


# --------------------------------------------------------------------------------------------------- the compiler report
def test_dense_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed); the figures are in DESIGN.md 4.16"""
    from test_kernel_resources import resources

    res = resources("ttx_dense.hip")
    names = sorted(k for k in res if "dense_" in k)
    for w in ("dense_fwd_kernelILi4ELi0", "dense_fwd_kernelILi4ELi1", "dense_fwd_kernelILi4ELi2", "dense_fwd_kernelILi1ELi0",
              "dense_fwd_kernelILi1ELi1", "dense_fwd_kernelILi1ELi2", "dense_keys_kernel", "dense_psw_grad_kernelILi4",
              "dense_psw_grad_kernelILi1", "dense_partial_kernelILi4", "dense_partial_kernelILi1", "dense_apply_kernelILi4",
              "dense_apply_kernelILi1"):
        assert sum(w in k for k in names) == 1, (w, names)
    assert len(names) == 13, names
    for k in names:
        print(k, res[k])
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["VGPRs"] <= 128 and res[k]["Occupancy"] >= 4, (k, res[k])
