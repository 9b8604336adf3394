"""tests/t4_ref.py, the host mirror of the four-core route's choices, held on the CPU: against the library's SOURCES (the route's
constants, t4_seg's thresholds, the merge's form and segment, t4_mfma and the helpers' cut-offs, t4_lds, t4_grid's cap, the apply
kernel's block and row-group arithmetic, the ids of include/ttx_test_hooks.h) and -- the condition that keeps
tests/test_t4_routes_gpu.py honest -- its case table against the mirror: every value of every field of t4_ref.route() is taken by
some case, and every geometry merges onto the template the table names.  Moving a threshold fails here until the mirror follows;
the GPU tests then compare the mirror with what the library's host code reports it chose (ttx_debug_t4_route)."""
import os
import re

import spec_ref as SR
import t4_ref as T4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "fbtt-embedding_amd", "csrc", "ttx_tt.hip")) as f:
    TT = f.read()
with open(os.path.join(ROOT, "include", "ttx_test_hooks.h")) as f:
    HOOKS = f.read()
SQ = re.sub(r"\s+", "", re.sub(r"\\\n", "", TT))  # (spaces squeezed, macro continuations joined)


def _const(name):
    m = re.findall(rf"constexpr int {name} = (\d+);", TT)
    assert len(m) == 1, f"{name}: {len(m)} definitions"
    return int(m[0])


def _has(text, what):
    assert SQ.count(re.sub(r"\s+", "", text)) >= 1, f"{what} is no longer `{text}`"


def _define(name):
    m = re.findall(rf"^#define {name} (\d+)\b", HOOKS, flags=re.M)
    assert len(m) == 1, f"{name}: {len(m)} definitions"
    return int(m[0])


def test_constants_are_the_sources():
    assert _const("kT4Slice") == SR.T4_SLICE and _const("kT4Stage") == SR.T4_STAGE
    assert _const("kT4Batch") == T4.T4_BATCH and _const("kT4Threads") == T4.T4_THREADS
    _has("constexpr int kT4ApplyBlock = 4 * kT4Threads;", "kT4ApplyBlock")
    assert T4.T4_APPLY_BLOCK == 4 * T4.T4_THREADS
    assert _const("kT4MSeg") == max(T4.merge_seg(n) for n in (1, 1 << 15, 1 << 17, 1 << 30))  # (the sorted merge's static record array)


def test_thresholds_are_the_sources():
    _has("return nnz >= (1 << 18) ? 128 : (nnz >= (1 << 16) ? 64 : (nnz >= (1 << 14) ? 32 : 16));", "t4_seg")
    _has("const int seg = nnz >= (1 << 17) ? 32 : (nnz >= (1 << 15) ? 16 : 4);", "the sorted merge's seg")
    _has("if (d.r[3] <= 32 && r2q2 <= 256 && !old_form) {", "the sorted-form condition")
    _has("const int threads = (r2q2 + 63) / 64 * 64;", "the sorted merge's block")
    _has("dim3((unsigned)((nnz + seg - 1) / seg)), dim3(threads), lds, st, P, c2, c3, P.t4m, r2q2, d.r[3], seg, reuse)", "the sorted merge's launch")
    _has("hipLaunchKernelGGL(t4_merge_kernel<Q>, dim3(t4_grid(nnz * r2q2)), dim3(256)", "the per-lookup merge's launch")
    _has("const long long b = (work + 255) / 256; return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));", "t4_grid")
    assert T4.T4_GRID_CAP == 16384
    _has("const bool t4_mfma = !t4_valu && r2q2 % 16 == 0 && d.r[3] % 16 == 0 && n2 / 256 <= 32;", "t4_mfma")
    _has("if (n2 / 256 <= 16) {", "the MFMA helper's cut-off")
    assert SQ.count("if(n2<=8*kT4Threads)hipLaunchKernelGGL((t4_grad23_kernel<Q,8>)") == 1
    assert SQ.count("elseif(n2<=16*kT4Threads)hipLaunchKernelGGL((t4_grad23_kernel<Q,16>)") == 1
    assert SQ.count("elsehipLaunchKernelGGL((t4_grad23_kernel<Q,32>)") == 1
    assert SQ.count("hipLaunchKernelGGL((t4_grad23_mfma_kernel<Q,4>)") == 1 and SQ.count("}else{if(lds_m>64*1024){rc=allow_lds(t4_grad23_mfma_kernel<Q,8>") == 1
    _has("const size_t lds = (size_t)((n2 + 3) / 4 * 4 + kT4Batch * (pm + n3)) * sizeof(float);", "the VALU helper's LDS")
    _has("if (lds > 64 * 1024) {", "the VALU helper's LDS opt-in")
    _has("if (lds_m > 64 * 1024) { rc = allow_lds(t4_grad23_mfma_kernel<Q, 4>, (int)lds_m);", "the MFMA helper's LDS opt-in")
    assert T4.LDS_OPT_IN == 64 * 1024
    # t4_lds
    _has("L.pmS = (q3 == 2 || q3 == 4 || q3 == 8) ? pm + (((2 * q3 - pm) % 32) + 32) % 32 : (pm + 3) / 4 * 4;", "t4_lds pmS")
    _has("L.r3S = r3 + (((16 - r3) % 32) + 32) % 32;", "t4_lds r3S")
    _has("L.oG = r2q2 * L.r3S; L.oC = L.oG + kT4Batch * L.pmS; L.floats = L.oC + kT4Batch * r3 * q3;", "t4_lds floats")
    # one SEG for the helper and the apply; the helper's grid
    _has("const int SEG = t4_seg(nnz);", "the helper's SEG")
    _has("const int gblocks = (int)((nnz + SEG - 1) / SEG);", "the helper's grid")
    _has("d.slice[2], d.slice[3], t4_seg(nnz), optim, lr, eps,", "the apply's SEG")
    # the apply kernel: blocks of a core-2 slice, where it looks for the partial rows, the core-3 row groups
    _has("const int nb2 = (n2 + kT4ApplyBlock - 1) / kT4ApplyBlock;", "nb2")
    _has("dim3(d.S[2] * ((d.slice[2] + kT4ApplyBlock - 1) / kT4ApplyBlock) + d.S[3]), dim3(kT4Threads)", "the apply's grid")
    _has("const int r1 = (beg / SEG + 1) * SEG;", "the first partial row behind a slice's own")
    _has("for (; r + 3 * SEG < end; r += 4 * SEG) {", "the four-rows-in-flight loop")
    _has("for (int e0 = 0; e0 < sl; e0 += kT4Threads) { const int V = min(sl - e0, kT4Threads), G = kT4Threads / V;", "the core-3 passes")
    _has("for (; r + 7 * G < end; r += 8 * G) {", "the eight-rows-in-flight loop")
    # Q3: an instantiation per value
    _has("case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; "
         "case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;", "TTX_T4_Q3")


def test_record_ids_are_the_header():
    for h, i in T4.HELPER_ID.items():
        assert _define("TTX_T4_HELPER_" + h.upper()) == i
    assert _define("TTX_T4_MERGE_SORTED") == T4.FORM_ID[T4.SORTED] and _define("TTX_T4_MERGE_PER_LOOKUP") == T4.FORM_ID[T4.PER_LOOKUP]
    import tt_embeddings as E

    names = ("MERGE_FORM", "MERGE_SEG", "MERGE_GRID", "SEG", "HELPER", "LDS_BYTES", "LDS_OPT_IN", "APPLY_SEG", "HELPER_Q3")
    assert [_define("TTX_T4_" + n) for n in names] == list(range(len(names))) and _define("TTX_T4_ROUTE_INTS") == len(names)
    assert E.T4_ROUTE_FIELDS == tuple(n.lower().replace("helper_q3", "q3") for n in names)
    # the record is written under TTX_TEST_HOOKS only
    assert SQ.count("#ifdefTTX_TEST_HOOKS//(ttx_debug_t4_route") == 1 and "#define TTX_T4_ROUTE(k, v) ((void)0)" in TT
    assert len(re.findall(r"ttx_debug_t4_route", re.sub(r"//[^\n]*", "", TT))) == 2, "the macro and the definition, nothing else"


def test_mirror_on_hand_written_cases():
    assert [T4.seg(n) for n in (1, 16383, 16384, 65535, 65536, 262143, 262144)] == [16, 16, 32, 32, 64, 64, 128]
    assert [T4.merge_seg(n) for n in (1, 32767, 32768, 131071, 131072)] == [4, 4, 16, 16, 32]
    assert T4.route([4, 4, 4, 16], [16, 16, 16], 100) is None
    r = T4.route([4, 4, 4, 4], [32, 32, 32], 10240)   # the default four-core factoring of D = 256
    assert (r["merge"], r["merge_seg"], r["merge_threads"], r["SEG"], r["helper"], r["Q3"], r["nb2"], r["core3"]) == \
        (T4.SORTED, 4, 128, 16, "mfma4", 4, 4, [(128, 2)])
    assert r["lds_bytes"] == 4 * (128 * 48 + 16 * 520 + 16 * 128) == 66048 and r["lds_opt_in"]  # (512 B above the opt-in)
    r = T4.route([4, 4, 4, 8], [16, 30, 40], 300)
    assert (r["merge"], r["helper"], r["lds_bytes"], r["lds_opt_in"], r["core3"]) == (T4.PER_LOOKUP, "valu32", 101120, True, [(256, 1), (64, 4)])
    assert T4.core3_passes(300) == [(256, 1), (44, 5)] and T4.core3_passes(384) == [(256, 1), (128, 2)] and T4.core3_passes(8) == [(8, 32)]
    # r2 q2 = 32: 131,072 lookups are exactly t4_grid's 16,384 work-groups of 256 (lookup, row) pairs; one more lookup strides
    assert not T4.route([2, 2, 2, 2], [16, 16, 48], 1 << 17)["grid_wraps"] and T4.route([2, 2, 2, 2], [16, 16, 48], (1 << 17) + 1)["grid_wraps"]
    assert T4.route([2, 2, 2, 2], [16, 16, 48], 1 << 18)["grid_wraps"]
    assert T4.run_counts(16) == [16, 1, 15, 17, 0, 83, 2, 0] and sum(T4.run_counts(16)) % 16 != 0
    assert sum(T4.run_counts(64, 65535)) == 65535 and T4.run_counts(64, 65535)[6] == 32767
    assert T4.core3_counts(134, 8) == [1, 0, 65, 34, 34] and sum(T4.core3_counts(16383, 32)) == 16383


def _records():
    """every launch geometry of the GPU file's table -> (what, record)"""
    out = [(f"a:{name}", T4.route(q, ranks, T4.SMALL_NNZ)) for name, (q, ranks, _, _) in T4.INSTANCES.items()]
    for name, (q, ranks) in T4.SWITCH.items():
        for k in T4.SWITCH_K:
            out += [(f"c:{name} 2^{k}-1", T4.route(q, ranks, (1 << k) - 1)), (f"c:{name} 2^{k}", T4.route(q, ranks, 1 << k))]
    return out


def test_every_geometry_merges_onto_the_template_the_table_names():
    for name, (q, ranks, template, _) in T4.INSTANCES.items():
        m = SR.t4_merged(q, ranks)
        assert m is not None, f"{name}: q = {q}, ranks {ranks} does not take the four-core route"
        assert SR.spec_match(*m)[0] == template == T4.route(q, ranks, 1)["template"], f"{name}: {SR.spec_match(*m)}"
    for name, (q, ranks) in T4.SWITCH.items():
        assert SR.t4_merged(q, ranks) is not None and SR.match_any(q, ranks) == ("S2_16_2_16_4", False), name
        assert int(q[0] * q[1] * q[2] * q[3]) == 16
    assert all(n in T4.INSTANCES for n in T4.STRUCT)
    assert len(T4.P4) == 4 and len(T4.SWITCH_P) == 4 and len(T4.STRUCT_P) == 4 and T4.SWITCH_P[2] == T4.STRUCT_P[2] == len(T4.run_counts(16))


def test_case_table_covers_every_value_of_every_field():
    recs = _records()
    assert all(r is not None for _, r in recs)
    a = [r for w, r in recs if w.startswith("a:")]
    c = [r for w, r in recs if w.startswith("c:")]
    assert {r["helper"] for r in a} == set(T4.HELPERS), "a gradient helper instantiation without a case"
    assert any(r["lds_opt_in"] and r["helper"].startswith("mfma") for r in a) and any(r["lds_opt_in"] and r["helper"].startswith("valu") for r in a)
    assert any(not r["lds_opt_in"] for r in a)
    for kernel in T4.TEMPLATED:
        got = {r["Q3"] for r in a if kernel in T4.kernels(r)}
        assert got == set(range(1, 9)), f"{kernel}: no case with Q3 in {sorted(set(range(1, 9)) - got)}"
    assert {r["merge"] for r in a} == {T4.SORTED, T4.PER_LOOKUP} == {r["merge"] for r in c}
    assert {r["merge_seg"] for r in c if r["merge"] == T4.SORTED} == {4, 16, 32}
    assert {r["SEG"] for r in c} == {16, 32, 64, 128}
    # both sides of every threshold, under both helper families and the per-lookup merge
    for name, (q, ranks) in T4.SWITCH.items():
        for k, lo, hi in ((14, 16, 32), (16, 32, 64), (18, 64, 128)):
            assert (T4.route(q, ranks, (1 << k) - 1)["SEG"], T4.route(q, ranks, 1 << k)["SEG"]) == (lo, hi)
        if T4.route(q, ranks, 1)["merge"] == T4.SORTED:
            for k, lo, hi in ((15, 4, 16), (17, 16, 32)):
                assert (T4.route(q, ranks, (1 << k) - 1)["merge_seg"], T4.route(q, ranks, 1 << k)["merge_seg"]) == (lo, hi)
    fam = {(T4.route(q, r, 1)["merge"], T4.route(q, r, 1)["helper"]) for q, r in T4.SWITCH.values()}
    assert fam == {(T4.SORTED, "mfma4"), (T4.SORTED, "valu8"), (T4.PER_LOOKUP, "mfma4")}
    assert any(r["grid_wraps"] for r in c) and any(r["merge"] == T4.PER_LOOKUP and not r["grid_wraps"] for r in c)
    assert any(r["merge_threads"] == 64 for r in a) and any(r["merge_threads"] > 64 for r in a if r["merge"] == T4.SORTED)
    # the apply kernel
    assert any(r["nb2"] == 1 for r in a) and any(r["nb2"] > 1 and r["n2"] % T4.T4_APPLY_BLOCK != 0 for r in a)
    assert any(r["nb2"] == 8 for r in a), "a core-2 slice of kT4Slice floats"
    assert any(r["n3"] < 256 and 256 % r["n3"] == 0 for r in a), "a core-3 slice that divides 256"
    assert any(r["n3"] < 256 and 256 % r["n3"] != 0 for r in a), "a core-3 slice below 256 that does not divide it"
    assert any(len(r["core3"]) == 2 and r["core3"][1][0] < 256 for r in a), "a core-3 slice above 256 with a remainder pass"
    assert any(len(r["core3"]) == 2 and 256 % r["core3"][1][0] != 0 for r in a), "a remainder pass with idle lanes"
    assert any(len(r["core3"]) == 4 for r in a), "a core-3 slice of several whole passes"
    # vector and scalar forms of the merge's loads; both ways the VALU helper maps threads onto (row, k)
    assert any(r["merge"] == T4.PER_LOOKUP and (r["n3"] // r["Q3"]) % 4 for r in a) and any(r["merge"] == T4.SORTED and (r["n3"] // r["Q3"]) % 4 for r in a)
    valu = [r for r in a if r["helper"].startswith("valu")]
    assert any(256 % (r["n3"] // r["Q3"]) == 0 for r in valu) and any(256 % (r["n3"] // r["Q3"]) != 0 for r in valu)
    # the run-structure cases: both helper families and a core-3 slice of two passes, at SEG = 16
    s = [T4.route(*T4.INSTANCES[n][:2], sum(T4.run_counts(16))) for n in T4.STRUCT]
    assert all(r["SEG"] == 16 for r in s) and {r["helper"][:4] for r in s} == {"mfma", "valu"} and any(len(r["core3"]) == 2 for r in s)
    assert T4.merge_seg(T4.REUSE_NNZ) == 16 and T4.route(*T4.SWITCH["sorted_mfma4"], T4.REUSE_NNZ)["merge"] == T4.SORTED
