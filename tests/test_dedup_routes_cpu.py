"""tests/dedup_ref.py, the host reference of the duplicate-lookup route, held on the CPU: against inputs whose map is written out by
hand, against the library's SOURCES (every constant and dispatch condition it mirrors), and -- the condition that keeps
tests/test_dedup_routes_gpu.py honest -- that file's case tables against dedup_ref.route / gsum_layout: every value of every choice
is expected by at least one case, every threshold has a case on each side, and every run / bag layout holds what its name says.

kDedupMaxTables together with plan_groups_tables: REACHABLE in a batch a test can afford.  tstart is written for
1 < tables <= 1023 when the largest count of slice ids, tables * max(p), is beyond 4096; 1023 tables of p = [5, 6, 5] have 5115 slice ids
in core 0, 1024 have 5120 and no room in the header -- the cores of such tables are never allocated by the map-only cases
(tables-1023 | tables-1024 of the GPU file, 3000 lookups each)."""
import os
import re

import numpy as np

import dedup_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")


# ---- the definition, by hand -------------------------------------------------------------------------------------------------------
def test_expected_map_on_a_hand_written_batch():
    """two tables of p = [2, 3] (6 rows each): keys 5 6 5 5 6 8 after the clamps -- index 7 is the last row, -1 is row 0, table 5 is table 1"""
    m = DR.expected_map(2, [2, 3], [5, 0, 5, 7, -1, 2], [0, 1, 0, 0, 1, 5])
    assert m["keys"].tolist() == [5, 6, 5, 5, 6, 8]
    assert m["nu"] == 3 and m["uidx"].tolist() == [5, 0, 2] and m["utab"].tolist() == [0, 1, 1]
    assert m["uid"].tolist() == [0, 1, 0, 0, 1, 2]
    assert m["occ"].tolist() == [0, 2, 3, 1, 4, 5], "a pair's occurrences in index order"
    assert m["occ_off"].tolist() == [0, 3, 5, 6] and m["iota"].tolist() == [0, 1, 2, 3, 4, 5]
    assert m["tstart"].tolist() == [0, 1, 3]
    assert (m["uid"].dtype, m["occ"].dtype, m["occ_off"].dtype, m["uidx"].dtype, m["iota"].dtype) == (np.int32,) * 3 + (np.int64,) * 2
    # one table: tableidx is not looked at; no duplicates: the identity
    one = DR.expected_map(1, [2, 3], [3, 1, 3], [9, -9, 4])
    assert one["keys"].tolist() == [3, 1, 3] and one["nu"] == 2 and one["occ"].tolist() == [1, 0, 2] and one["tstart"].tolist() == [0, 2]
    ident = DR.expected_map(1, [4, 4], np.arange(16), None)
    assert ident["nu"] == 16 and np.array_equal(ident["occ"], np.arange(16)) and np.array_equal(ident["uid"], np.arange(16))
    # a table without a lookup: its group is empty
    assert DR.expected_map(4, [2, 3], [1, 1, 2], [3, 1, 1])["tstart"].tolist() == [0, 0, 2, 2, 3]
    # exactly 2^32 keys: the largest key has every bit, the clamp holds it there
    big = DR.expected_map(2, [2048, 1024, 1024], [(1 << 31) - 1, 1 << 31, 0, -1], [1, 1, 1, 0])
    assert big["keys"].tolist() == [(1 << 32) - 1, (1 << 32) - 1, 1 << 31, 0] and big["uidx"].tolist() == [0, 0, (1 << 31) - 1]


def test_carve_on_a_hand_written_size():
    lay = DR.carve(100)     # n = r64(101) = 128 entries; the header is 64 + 1024 * 8 = 8256 bytes -> 8448
    assert DR.DEDUP_HDR_BYTES == 8256
    assert {k: v[0] for k, v in lay.items() if k != "map_bytes"} == dict(nu=0, tstart=64, uidx=8448, utab=9472, iota=10496, uid=11520,
                                                                       occ=12032, occ_off=12544)
    assert lay["map_bytes"] == 13056
    assert DR.carve(63)["utab"][0] - DR.carve(63)["uidx"][0] == 512 and DR.carve(64)["utab"][0] - DR.carve(64)["uidx"][0] == 1024


def test_route_on_hand_written_shapes():
    r = DR.route(1, [7, 6, 5], 100, 16)
    assert r == dict(form=DR.SMALL, bpw=2, passes=1, nblk=0, tstart=0, pool=DR.POOL_GATHER_VEC4, gsum=DR.VEC4)
    assert [DR.small_nb(n) for n in (1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384)] == [1, 1, 2, 2, 3, 4, 5, 8, 9, 12, 13, 16]
    assert [DR.route(1, [7, 6, 5], n, 16)["bpw"] for n in (2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384)] == [2, 4, 4, 8, 8, 12, 12, 16, 16]
    assert DR.route(1, [7, 6, 5], 16385, 16) == dict(form=DR.LARGE, bpw=0, passes=1, nblk=17, tstart=0, pool=DR.POOL_GATHER_VEC4, gsum=DR.VEC4)
    for keys, passes in ((256, 1), (257, 2), (1 << 16, 2), ((1 << 16) + 1, 3), (1 << 24, 3), ((1 << 24) + 1, 4), (1 << 32, 4)):
        assert (DR._bits(keys, DR.SMALL_BITS_CAP) + 7) // 8 == passes
    assert DR.route(2, [2048, 1024, 1024], 100, 16)["form"] == DR.SMALL and DR.route(3, [2048, 1024, 1024], 100, 16)["form"] == DR.LARGE
    assert DR.route(1, [2048, 2048, 1024], 100, 16)["form"] == DR.SMALL and DR.route(1, [2048, 2048, 1025], 100, 16)["form"] == DR.LARGE
    assert DR.route(2, [1 << 20, 1 << 20, (1 << 20) - 1], 100, 16)["passes"] == 8 and not DR.supported(2, [1 << 20, 1 << 20, (1 << 20) + 1], 100)
    assert not DR.supported(1, [7, 6, 5], 0) and DR.supported(1, [7, 6, 5], (1 << 31) - 1) and not DR.supported(1, [7, 6, 5], 1 << 31)
    # pooling and pre-sum
    assert DR.route(1, [7, 6, 5], 65536, 16)["pool"] == DR.POOL_GATHER_VEC4 and DR.route(1, [7, 6, 5], 65537, 16)["pool"] == DR.POOL_SPAN
    assert DR.route(1, [7, 6, 5], 65537, 18)["pool"] == DR.POOL_GATHER_SCALAR and DR.route(1, [7, 6, 5], 100, 16, pool_aligned=False)["pool"] == DR.POOL_GATHER_SCALAR
    assert DR.route(1, [7, 6, 5], 100, 16, aligned=False, pool_aligned=True) == dict(form=DR.SMALL, bpw=2, passes=1, nblk=0, tstart=0,
                                                                                    pool=DR.POOL_GATHER_VEC4, gsum=DR.SCALAR)
    assert DR.route(1, [7, 6, 5], 100, 15)["gsum"] == DR.SCALAR
    # tstart
    assert [DR.route(tb, p, n, 16)["tstart"] for tb, p, n in ((1, [5000, 6, 5], 100), (4, [64, 6, 5], 100), (16, [256, 6, 5], 100), (17, [241, 6, 5], 100),
                                                            (2, [200, 6, 5], 393216), (2, [200, 6, 5], 393217), (1023, [5, 6, 5], 100),
                                                            (1024, [5, 6, 5], 100))] == [0, 0, 0, 1, 0, 1, 1, 0]
    assert [DR.scan_trips(n) for n in (1, 1 << 20, (1 << 20) + 1)] == [1, 1, 2]


def test_gsum_layout_on_hand_written_runs():
    lay = DR.gsum_layout([0, 5, 32, 64, 100, 100 + 64 * 32, 100 + 64 * 32 + 2], 100 + 64 * 32 + 2)
    assert lay["first"].tolist() == [0, 0, 1, 2, 3, 67] and lay["last"].tolist() == [0, 0, 1, 3, 67, 67]
    assert lay["kind"].tolist() == [DR.IN_SLICE, DR.IN_SLICE, DR.IN_SLICE, DR.FOLD_ONE, DR.FOLD_COOP, DR.IN_SLICE]   # [100, 2148): slices 3..67 = 65
    assert lay["wg"].tolist() == [0, 0, 0, 0, 4, 4]


def test_presum_feeds_the_backward_of_the_distinct_pairs():
    """Gu, stated in occ order, is what the backward of the DISTINCT pairs consumes: the pairs as a batch of their own (one bag each,
    bag gradient Gu[u]) have the gradients of the whole batch -- in float64 to rounding"""
    import gen_inputs as G
    import tt_ref64 as R

    tables, p, q, r, B = 2, [3, 4, 2], [2, 3, 2], [1, 4, 5, 1], 5
    rs = np.random.RandomState(3)
    N = 60
    idx, tb = rs.randint(0, 24, size=N), np.sort(rs.randint(0, 2, size=N))
    row = rs.randint(0, B, size=N)
    w = rs.rand(N) + 0.5
    cores = G.make_cores(1, tables, p, q, r, "signed")
    d_out = G.make_grad(2, tables, B, 12)
    m = DR.expected_map(tables, p, idx, tb)
    assert m["nu"] < N
    for psw in (None, w):
        Gu = DR.presum64(m, row, tb, B, d_out, psw)
        # by hand for one pair
        u = int(np.argmax(np.diff(m["occ_off"])))
        occ = m["occ"][m["occ_off"][u]:m["occ_off"][u + 1]]
        assert (np.diff(occ) > 0).all() and len(occ) > 1
        by_hand = sum((1.0 if psw is None else psw[n]) * d_out[tb[n], row[n]].astype(np.float64) for n in occ)
        assert np.allclose(Gu[u], by_hand, rtol=1e-14, atol=0)
        whole = R.forward_backward(tables, p, q, r, B, idx, row, tb, cores, d_out, per_sample_weights=psw)
        nu = m["nu"]
        gd = np.zeros((tables, nu, 12))
        gd[m["utab"], np.arange(nu)] = Gu
        pairs = R.forward_backward(tables, p, q, r, nu, m["uidx"], np.arange(nu), m["utab"], cores, gd)
        for a, b in zip(whole["grads"], pairs["grads"]):
            assert np.allclose(a, b, rtol=1e-12, atol=1e-15)


# ---- the constants and conditions, pinned to the sources ------------------------------------------------------------------------------
def _squeeze(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"\\\n", "", text)
    return re.sub(r"\s+", "", text)


def _constexpr(text, name, typ="int"):
    m = re.search(r"constexpr\s+" + typ + r"\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, f"constexpr {typ} {name} not found"
    return m.group(1).strip()


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_map_constants_and_choices_match_the_sources():
    """dedup_ref.carve / route restate carve_dedup, dedup_supported, dedup_build, dedup_build_map, dedup_build_large and
    plan_groups_tables: a retuned constant or a changed condition must fail HERE until the mirror follows"""
    plan, internal = _src("ttx_plan.hip"), _src("ttx_internal.h")
    sq, sqi = _squeeze(plan), _squeeze(internal)
    assert int(_constexpr(internal, "kWave")) == DR.WAVE
    assert int(_constexpr(internal, "kDedupMaxN")) == DR.DEDUP_MAX_N
    assert int(_constexpr(plan, "kPlanThreads")) == DR.PLAN_THREADS and _constexpr(plan, "kPlanWaves") == "kPlanThreads / kWave"
    assert int(_constexpr(plan, "kDdThreads")) == DR.DD_THREADS
    assert int(_constexpr(plan, "kDedupMaxTables")) == DR.DEDUP_MAX_TABLES
    assert _constexpr(plan, "kDedupHdrBytes", "size_t") == "64 + (kDedupMaxTables + 1) * sizeof(int64_t)"
    assert DR.DEDUP_HDR_BYTES == 64 + (DR.DEDUP_MAX_TABLES + 1) * 8
    assert f"inlinesize_talign_up(size_tx,size_ta={DR.ALIGN}){{return(x+a-1)/a*a;}}" in sqi
    assert "staticsize_tr64(size_tk){return(k+63)/64*64;}" in sq
    assert f"inlineint64_t*dedup_tstart(constDedupMap&M){{return(int64_t*)((char*)M.nu+{DR.TSTART_BYTE});}}" in sqi
    # carve_dedup: the order and the element sizes of the arrays
    assert ("DedupMapcarve_dedup(longlongnnz,void*base){constsize_tn=r64((size_t)nnz+1);char*cur=(char*)base;"
            "autotake=[&](size_tbytes){char*r=cur;cur+=align_up(bytes);returnr;};DedupMapM;M.nu=(int*)take(kDedupHdrBytes);"
            "M.uidx=(int64_t*)take(n*sizeof(int64_t));M.utab=(int64_t*)take(n*sizeof(int64_t));M.iota=(int64_t*)take(n*sizeof(int64_t));"
            "M.uid=(int*)take(n*sizeof(int));M.occ=(int*)take(n*sizeof(int));M.occ_off=(int*)take(n*sizeof(int));returnM;}") in sq
    assert "returnalign_up(kDedupHdrBytes)+3*align_up(n*sizeof(int64_t))+3*align_up(n*sizeof(int));" in sq
    assert f"staticsize_tdedup_blocks(longlongnnz){{return((size_t)nnz+{DR.DD_BLOCK - 1})/{DR.DD_BLOCK};}}" in sq
    # which batches are mapped, and by which form
    assert "if(d.tab||!d.idx32)return0;" in sq
    assert f"return(e<=(1ull<<{DR.SMALL_KEY_BITS})&&all<=(1ull<<{DR.SMALL_KEY_BITS}))?all:0;" in sq
    assert f"if(e>(1ull<<{DR.LARGE_KEY_BITS})/(unsignedlonglong)d.p[t])return0;" in sq
    assert f"if(e>(1ull<<{DR.LARGE_KEY_BITS})/(unsignedlonglong)d.num_tables)return0;returne*(unsignedlonglong)d.num_tables;" in sq
    assert ("booldedup_supported(constDims&d,longlongnnz){if(nnz<=0||nnz>=(1ll<<31))returnfalse;"
            "if(nnz<=kDedupMaxN&&dedup_key_space(d)!=0)returntrue;returndedup_key_space64(d)!=0;}") in sq
    api = _squeeze(_src("ttx_api.hip"))
    assert "d->idx32=Lv<=(1ll<<32);" in api
    # dedup_build_map, in its order: the large form; the passes; nb; the ladder
    marks = [
        "staticintdedup_build_map(constDims&d,longlongnnz,constint64_t*indices,constint64_t*tableidx,constDedupMap&M,hipStream_tstream){",
        "if(nnz>kDedupMaxN||dedup_key_space(d)==0)returndedup_build_large(d,nnz,indices,tableidx,M,stream);",
        "constunsignedlonglongall=dedup_key_space(d);",
        f"intbits=1;while(bits<{DR.SMALL_BITS_CAP}&&(1ull<<bits)<all)++bits;constintpasses=(bits+7)/8;",
        "constintper=((N+kPlanWaves-1)/kPlanWaves+kWave-1)/kWave*kWave;constintnb=per/kWave;",
        "TTX_DD_ROUTE(TTX_DD_FORM,TTX_DD_SMALL),TTX_DD_ROUTE(TTX_DD_PASSES,passes),TTX_DD_ROUTE(TTX_DD_NBLK,0);",
        "TTX_DD_ROUTE(TTX_DD_BPW,BPW);hipLaunchKernelGGL(dedup_small_kernel<BPW>,dim3(1),dim3(kPlanThreads),lds,stream,N,E,d.num_tables,passes,indices,tableidx,M);",
        "".join(f"{'else' if i else ''}if(nb<={b})TTX_DEDUP_LAUNCH({b});" for i, b in enumerate(DR.BPW_LADDER[:-1])) + f"elseTTX_DEDUP_LAUNCH({DR.BPW_LADDER[-1]});",
    ]
    at = 0
    for mk in marks:
        nxt = sq.find(mk, at)
        assert nxt >= 0, f"dedup_build_map no longer reads `{mk}` (in this order): update tests/dedup_ref.py::route"
        at = nxt
    assert sorted(set(int(x) for x in re.findall(r"TTX_DEDUP_LAUNCH\((\d+)\)", plan))) == sorted(DR.BPW_LADDER)
    # dedup_build_large
    marks = [
        "staticintdedup_build_large(",
        "constunsignedlonglongall=dedup_key_space64(d);",
        f"intbits=1;while(bits<{DR.LARGE_BITS_CAP}&&(1ull<<bits)<all)++bits;constintpasses=(bits+7)/8;",
        "constintnblk=(int)dedup_blocks(nnz);",
        "TTX_DD_ROUTE(TTX_DD_FORM,TTX_DD_LARGE),TTX_DD_ROUTE(TTX_DD_BPW,0),TTX_DD_ROUTE(TTX_DD_PASSES,passes),TTX_DD_ROUTE(TTX_DD_NBLK,nblk);",
        "hipLaunchKernelGGL(dd_keys_kernel,dim3(nblk),dim3(kDdThreads),",
        "sort_pairs_desc(nnz,keys,vals,sws,&sk,&sv,stream,passes);",
        "hipLaunchKernelGGL(dd_count_kernel,dim3(nblk),dim3(kDdThreads),",
        "hipLaunchKernelGGL(dd_scan_kernel,dim3(1),dim3(kDdThreads),0,stream,nblk,N,blk,M);",
        "hipLaunchKernelGGL(dd_emit_kernel,dim3(nblk),dim3(kDdThreads),",
    ]
    at = 0
    for mk in marks:
        nxt = sq.find(mk, at)
        assert nxt >= 0, f"dedup_build_large no longer reads `{mk}` (in this order): update tests/dedup_ref.py::route"
        at = nxt
    assert "for(intb0=0;b0<nblk;b0+=kDdThreads){" in sq, "dd_scan_kernel's trips over the block counts"
    assert "constinti=blockIdx.x*kDdThreads+threadIdx.x;" in sq
    # tstart: dedup_build's condition, and plan_groups_tables itself
    assert ("TTX_DD_ROUTE(TTX_DD_TSTART,0);if(d.num_tables<=kDedupMaxTables&&plan_groups_tables(d,nnz)){TTX_DD_ROUTE(TTX_DD_TSTART,1);"
            "ProfScopeps(TTX_PROF_PLAN,stream);hipLaunchKernelGGL(dedup_tstart_kernel,") in sq
    assert (f"boolplan_groups_tables(constDims&d,longlongN){{if(d.num_tables<=1||d.tab)returnfalse;intsmax=1;"
            f"for(intt=0;t<d.T;++t)if(d.S[t]>smax)smax=d.S[t];if(smax<={DR.ONE_DIGIT})returnfalse;"
            f"if(smax<={DR.WIDE_MAX_S}&&(N+kWideSpan-1)/kWideSpan<=kWideMaxG)returnfalse;returntrue;}}") in sq
    assert int(_constexpr(plan, "kWideThreads")) * int(_constexpr(plan, "kSB")) == DR.WIDE_SPAN and int(_constexpr(plan, "kWideMaxG")) == DR.WIDE_MAX_G
    # the clamps of both key kernels
    assert "constunsignedlonglonge=(unsignedlonglong)max(ix[b],0ll);constunsignedlonglongtb=(unsignedlonglong)min(max(tbv[b],0),num_tables-1);k[b]=(unsigned)(tb*E+(e<E?e:E-1));" in sq
    assert "tbv[b]=(tableidx&&num_tables>1)?(int)tableidx[i]:0;" in sq
    assert ("constunsignedlonglonge=(unsignedlonglong)max(indices[i],(int64_t)0);constinttbv=(tableidx&&num_tables>1)?(int)tableidx[i]:0;"
            "constunsignedlonglongtb=(unsignedlonglong)min(max(tbv,0),num_tables-1);") in sq
    assert "keys[i]=(int64_t)((unsignedlonglong)num_tables*E-1ull-(tb*E+(e<E?e:E-1)));" in sq


def test_pooling_and_presum_conditions_match_the_sources():
    tt, common = _src("ttx_tt.hip"), _src("ttx_tt_common.h")
    sq = _squeeze(tt)
    assert int(_constexpr(tt, "kPoolSpanMin")) == DR.POOL_SPAN_MIN and int(_constexpr(common, "kThreads")) == DR.THREADS
    assert int(_constexpr(tt, "kGsSlice")) == DR.GS_SLICE and int(_constexpr(tt, "kGsFoldCoop")) == DR.GS_FOLD_COOP
    assert int(_constexpr(tt, "kGsThreads")) == DR.GS_THREADS and _constexpr(tt, "kGsRounds") == "kGsSlice / 16"
    # ttx_tt_forward_dd: the three pooling kernels, in this order -- and the test library's record of the choice right in front of
    # the dispatch, under the SAME two conditions (the record restates them: the two texts are held together here)
    c_span = "if(d.D%4==0&&(((uintptr_t)rows|(uintptr_t)output)&15)==0&&nnz>kPoolSpanMin)"
    c_vec4 = "elseif(d.D%4==0&&(((uintptr_t)rows|(uintptr_t)output)&15)==0)"
    marks = [
        "intttx_tt_forward_dd(",
        "constintblocks=((int)nnz+kThreads/16-1)/(kThreads/16);#ifdefTTX_TEST_HOOKS"
        + c_span + "TTX_DD_ROUTE(TTX_DD_POOL,TTX_DD_POOL_SPAN);" + c_vec4 + "TTX_DD_ROUTE(TTX_DD_POOL,TTX_DD_POOL_GATHER_VEC4);"
        "elseTTX_DD_ROUTE(TTX_DD_POOL,TTX_DD_POOL_GATHER_SCALAR);#endif"
        + c_span + "hipLaunchKernelGGL(pool_gather4_kernel,dim3(((int)nnz+kThreads-1)/kThreads),dim3(kThreads),",
        c_vec4 + "hipLaunchKernelGGL(pool_gather_kernel<float4>,dim3(blocks),dim3(kThreads),",
        "elsehipLaunchKernelGGL(pool_gather_kernel<float>,dim3(blocks),dim3(kThreads),",
    ]
    at = 0
    for mk in marks:
        nxt = sq.find(mk, at)
        assert nxt >= 0, f"ttx_tt_forward_dd no longer reads `{mk}` (in this order): update tests/dedup_ref.py::route"
        at = nxt
    # gsum_launch_t: the vector type, the grid
    marks = [
        "staticintgsum_launch_t(",
        "constintblocks=((N+kGsSlice-1)/kGsSlice+kGsThreads/16-1)/(kGsThreads/16);",
        "if(D%4==0&&((((uintptr_t)d_output)|((uintptr_t)Gu))&15)==0){TTX_DD_ROUTE(TTX_DD_GSUM,TTX_DD_VEC4);hipLaunchKernelGGL((gsum_slice_kernel<float4,kSkip>),",
        "hipLaunchKernelGGL(gsum_fold_kernel<float4>,",
        "}else{TTX_DD_ROUTE(TTX_DD_GSUM,TTX_DD_SCALAR);hipLaunchKernelGGL((gsum_slice_kernel<float,kSkip>),",
        "hipLaunchKernelGGL(gsum_fold_kernel<float>,",
    ]
    at = 0
    for mk in marks:
        nxt = sq.find(mk, at)
        assert nxt >= 0, f"gsum_launch_t no longer reads `{mk}` (in this order): update tests/dedup_ref.py::route"
        at = nxt
    # what gsum_layout restates: a slice per 16-lane group, the group of the slice a run ENDS in folds it, the cooperative switch
    assert "constints=blockIdx.x*(kGsThreads/16)+threadIdx.x/16;constintk0=s*kGsSlice;if(k0>=N)return;" in sq
    assert "constintlo=M.occ_off[u],hi=M.occ_off[u+1];if((hi-1)/kGsSlice!=s)u=-1;elsesf=lo/kGsSlice;" in sq
    assert "if(u>=0&&s-sf+1>kGsFoldCoop){" in sq
    assert "constexprintkG=kGsThreads/16;" in sq and "constints=blockIdx.x*kG+g;" in sq
    # the backward hands the pre-sum d_output and the start of its workspace (Gu)
    assert "float*Gu=(float*)workspace;" in sq and "rc=gsum_launch(M,nnz,B,d.D,rowidx,tableidx,psw,d_output,Gu,(char*)workspace+gu_rows_bytes(d,nnz),st);" in sq
    # the ids of the record
    hooks = open(os.path.join(ROOT, "include", "ttx_test_hooks.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define\s+TTX_DD_([A-Z0-9_]+)\s+(\d+)", hooks)}
    assert ids == dict(FORM=0, BPW=1, PASSES=2, NBLK=3, TSTART=4, POOL=5, GSUM=6, ROUTE_INTS=len(DR.ROUTE_FIELDS), SMALL=DR.SMALL, LARGE=DR.LARGE,
                       POOL_GATHER_VEC4=DR.POOL_GATHER_VEC4, POOL_GATHER_SCALAR=DR.POOL_GATHER_SCALAR, POOL_SPAN=DR.POOL_SPAN, VEC4=DR.VEC4, SCALAR=DR.SCALAR)
    assert [k for k, v in sorted(ids.items(), key=lambda kv: kv[1]) if k in ("FORM", "BPW", "PASSES", "NBLK", "TSTART", "POOL", "GSUM")] == [f.upper() for f in DR.ROUTE_FIELDS]
    shim = open(os.path.join(ROOT, "fbtt-embedding_amd", "tt_embeddings.py")).read()
    assert re.search(r"DD_ROUTE_FIELDS\s*=\s*\(" + ",\\s*".join(f'"{f}"' for f in DR.ROUTE_FIELDS) + r"\)", shim)


# ---- the case tables of the GPU file -------------------------------------------------------------------------------------------------
def test_map_cases_stand_on_both_sides_of_every_threshold():
    import test_dedup_routes_gpu as GPU

    names = [c["name"] for c in GPU.MAP_CASES]
    assert len(set(names)) == len(names)
    routes = {c["name"]: GPU._rt(c) for c in GPU.MAP_CASES}
    for label, near, near_want, far, far_want in GPU.MAP_THRESHOLDS:
        for side, pred, want in (("near", near, near_want), ("far", far, far_want)):
            hit = [c for c in GPU.MAP_CASES if pred(c)]
            assert hit, f"{label}: no case on the {side} side"
            for c in hit:
                got = {k: routes[c["name"]][k] for k in want}
                assert got == want, f"{label}: case {c['name']} ({side} side) takes {got}, the table expects {want}"
    small = [r for r in routes.values() if r["form"] == DR.SMALL]
    large = [r for r in routes.values() if r["form"] == DR.LARGE]
    assert {r["bpw"] for r in small} == set(DR.BPW_LADDER) and {r["bpw"] for r in large} == {0}
    assert {r["passes"] for r in small} == {1, 2, 3, 4} and {1, 4, 5, 8} <= {r["passes"] for r in large}
    assert {r["tstart"] for r in routes.values()} == {0, 1}
    assert {DR.scan_trips(c["N"]) for c in GPU.MAP_CASES} == {1, 2}
    # the sizes the issue lists, and nothing above 10^5 lookups but the scan cases and the two that count the wide plan's work-groups
    assert {c["N"] for c in GPU.MAP_CASES if GPU._one(c)} == set(GPU.LADDER) == {1, 63, 64, 65, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385}
    assert sorted(c["name"] for c in GPU.MAP_CASES if c["N"] > 100000) == ["S-257-few-rows", "S-257-many-rows", "scan-1048576", "scan-1048577"]
    # key spaces: exactly the counts the names say
    keys = {c["name"]: c["tables"] * DR.rows_of(c["p"]) for c in GPU.MAP_CASES}
    assert [keys[n] for n in ("ks-2^8", "ks-2^8+1", "ks-2^16", "ks-2^16+1", "ks-2^24", "ks-2^24+1", "ks-2^32-two-tables", "ks-2^32-one-table")] == \
        [1 << 8, (1 << 8) + 1, 1 << 16, (1 << 16) + 1, 1 << 24, (1 << 24) + 1, 1 << 32, 1 << 32]
    assert keys["ks-3x2^31"] == 3 << 31 and keys["ks-64bit-100"] > 1 << 32 and (1 << 60) < keys["large-8-passes"] < 1 << 61
    assert not DR.supported(2, [1 << 20, 1 << 20, (1 << 20) + 1], 100), "large-8-passes is the last key space the library maps with these factors"
    # the make_dims limits the cases must respect: at most 2^30 slice ids per core
    assert all(c["tables"] * max(c["p"]) <= 1 << 30 for c in GPU.MAP_CASES)
    # every stream is used; the skewed ones meet the last size of the small form and the first of the large one
    assert {s for c in GPU.MAP_CASES for s in c["streams"]} == set(GPU.ALL_STREAMS)
    for n in ("n-65", "n-16384", "n-16385"):
        assert {"uniform", "same", "ends", "clamp"} <= set(next(c for c in GPU.MAP_CASES if c["name"] == n)["streams"])
    assert any(c["tables"] > 32 and routes[c["name"]]["tstart"] and "empty_tables" in c["streams"] for c in GPU.MAP_CASES), "a grouped case above 32 tables"


def test_map_streams_are_what_their_names_say():
    import test_dedup_routes_gpu as GPU

    by = {c["name"]: c for c in GPU.MAP_CASES}
    for name in ("n-65", "ks-2^32-two-tables", "tstart-7", "large-8-passes"):
        c = by[name]
        E = DR.rows_of(c["p"])
        for stream in c["streams"]:
            idx, tb = GPU.make_stream(c, stream)
            assert idx.size == tb.size == c["N"] and idx.dtype == tb.dtype == np.int64
            m = DR.expected_map(c["tables"], c["p"], idx, tb)
            if stream == "uniform":
                assert 1 < m["nu"] < c["N"], "duplicates and more than one pair"
            if stream == "same":
                assert m["nu"] == 1 and int(m["keys"][0]) == c["tables"] * E - 1
            if stream == "ends":
                assert set(m["uidx"].tolist()) == {0, E - 1} and m["nu"] == 2 * c["tables"]
            if stream == "empty_tables":
                cnt = np.diff(m["tstart"])
                assert cnt[0] == 0 and cnt[c["tables"] // 2] == 0 and cnt[-1] == 0 and (cnt > 0).sum() == c["tables"] - 3
            if stream == "clamp":
                assert (idx < 0).sum() >= 3 and (idx >= E).sum() >= 3 and (idx == E - 1).sum() >= 1 and (idx == 0).sum() >= 1
                last = m["keys"] == m["keys"][np.flatnonzero(idx >= E)[0]]
                assert len(set(idx[last].tolist())) >= 3, "several raw indices share the last row's pair only after the clamp"
                if c["tables"] > 1:
                    assert (tb < 0).any() and (tb >= c["tables"]).any()
    big = DR.expected_map(2, by["ks-2^32-two-tables"]["p"], *GPU.make_stream(by["ks-2^32-two-tables"], "ends"))
    assert int(big["keys"].max()) == (1 << 32) - 1 and (1 << 31) in big["keys"].tolist(), "the key of every bit, and the one negative as an int"
    d = by["distinct-16384"]
    assert DR.expected_map(1, d["p"], *GPU.make_stream(d, "distinct"))["nu"] == d["N"]
    # the scan cases: few pairs | a head in every block of 1024 sorted positions, the last (partial) one included
    c = by["scan-1048577"]
    m = DR.expected_map(1, c["p"], *GPU.make_stream(c, "heads"))
    heads = np.zeros(c["N"], dtype=bool)
    heads[m["occ_off"][:-1]] = True
    per_block = np.add.reduceat(heads, np.arange(0, c["N"], DR.DD_BLOCK))
    assert per_block.size == 1025 and (per_block > 0).all() and m["nu"] > 1 << 19
    assert DR.expected_map(1, c["p"], *GPU.make_stream(c, "few"))["nu"] == 5


def _layout(counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    return off, DR.gsum_layout(off, int(off[-1]))


def test_run_layouts_hold_the_runs_their_names_say():
    import test_dedup_routes_gpu as GPU

    S = DR.GS_SLICE
    off, lay = _layout(GPU.LAYOUTS["edges"])
    lo, hi, first, last, kind = off[:-1], off[1:], lay["first"], lay["last"], lay["kind"]
    assert off[-1] % S != 0 and off[-1] > S
    assert ((kind == DR.IN_SLICE) & (hi % S == 0) & (lo % S != 0)).any(), "a run inside a slice ending on position 31"
    assert ((kind == DR.IN_SLICE) & (lo % S == 0) & (hi - lo < S)).any(), "a run starting on position 0"
    assert ((lo % S == 0) & (hi - lo == S)).any(), "a run of exactly 32 on a slice"
    assert ((kind == DR.IN_SLICE) & (lo % S != 0) & (hi % S != 0)).any(), "a run strictly inside a slice"
    whole = (hi // S) - ((lo + S - 1) // S) - (hi % S == 0)     # whole slices strictly inside the run (not its last one)
    assert (whole >= 3).any(), "a run covering three whole slices strictly inside it"
    assert ((kind == DR.FOLD_ONE) & (hi % S == 0) & (lo % S != 0)).any(), "a crossing run that ends on the last position of a slice"
    assert ((kind == DR.FOLD_ONE) & (last - first == 1) & (hi % S != 0)).any(), "a short crossing run"
    assert ((kind == DR.FOLD_ONE) & (last - first == 2)).any()
    assert (kind == DR.FOLD_COOP).sum() == 0
    off, lay = _layout(GPU.LAYOUTS["tiny"])
    assert off[-1] < S and (lay["kind"] == DR.IN_SLICE).all()
    off, lay = _layout(GPU.LAYOUTS["long"])
    lo, hi, span = off[:-1], off[1:], lay["last"] - lay["first"] + 1
    assert off[-1] % S != 0
    i64, i65, i66 = (int(np.flatnonzero(span == n)[0]) for n in (64, 65, 66))
    assert (hi - lo)[[i64, i65, i66]].tolist() == [2048, 2049, 2050] and (lo % S)[[i64, i65, i66]].tolist() == [0, 0, 31]
    assert lay["kind"][[i64, i65, i66]].tolist() == [DR.FOLD_ONE, DR.FOLD_COOP, DR.FOLD_COOP]
    assert DR.GS_FOLD_COOP == 64, "64 | 65 slices stand on either side of the cooperative fold"
    short = np.flatnonzero((lay["kind"] == DR.FOLD_ONE) & (span == 2))
    assert short.size == 1 and lay["wg"][short[0]] == lay["wg"][i66] and lay["last"][short[0]] != lay["last"][i66], \
        "a cooperative and a short crossing run end in the same work-group of 16 slices"
    assert 6000 <= off[-1] <= 6300


def test_e2e_cases_expect_every_kernel():
    import test_dedup_routes_gpu as GPU

    names = [c["name"] for c in GPU.E2E_CASES]
    assert len(set(names)) == len(names)
    batches = {c["name"]: GPU.make_e2e(c) for c in GPU.E2E_CASES}
    routes = {c["name"]: GPU.e2e_route(c, batches[c["name"]]["N"]) for c in GPU.E2E_CASES}
    assert {r["pool"] for r in routes.values()} == {DR.POOL_GATHER_VEC4, DR.POOL_GATHER_SCALAR, DR.POOL_SPAN}
    assert {r["gsum"] for r in routes.values()} == {DR.VEC4, DR.SCALAR}
    assert {r["form"] for r in routes.values()} == {DR.SMALL, DR.LARGE}
    for c in GPU.E2E_CASES:
        b, r = batches[c["name"]], routes[c["name"]]
        assert int(np.prod(c["q"])) == c["D"] and b["indices"].size == b["N"] == b["offsets"][-1]
        assert (b["indices"] >= 0).all() and (b["indices"] < DR.rows_of(c["p"])).all()
        assert (np.diff(b["tableidx"]) >= 0).all(), "table-major bags"
        if c["layout"]:
            m = DR.expected_map(c["tables"], c["p"], b["indices"], b["tableidx"])
            assert np.array_equal(np.diff(m["occ_off"]), GPU.LAYOUTS[c["layout"]]), f"{c['name']}: the runs are the layout"
            assert b["N"] <= 6300
            if c["tables"] > 1:
                assert (np.diff(m["tstart"]) > 0).all(), "every table has pairs"
        if c["misaligned"]:
            assert c["D"] % 4 == 0 and r["gsum"] == DR.SCALAR and r["pool"] == DR.POOL_GATHER_VEC4
    for lname in GPU.LAYOUTS:   # every run layout at every D, misaligned, weighted, over three tables
        mine = [c for c in GPU.E2E_CASES if c["layout"] == lname]
        assert {16, 72, 128, 15, 18} <= {c["D"] for c in mine if not (c["misaligned"] or c["psw"] or c["tables"] > 1)}
        assert any(c["misaligned"] for c in mine) and any(c["psw"] for c in mine) and any(c["tables"] == 3 for c in mine)
    assert (72 // 4) % 16 != 0 and 72 // 4 > 16, "D = 72: a partial second block of 16 float4 columns"
    assert any(c["q"] == [4, 4, 4] and c["r"] == [1, 16, 16, 1] for c in GPU.E2E_CASES), "one specialised geometry"
    # pool_gather_kernel's bag layouts, in both vector types
    lens = GPU.POOL_BAGS
    assert {0, 1, 15, 16, 17, 32, 33} <= set(lens) and lens[0] == 0 and lens[-1] == 0 and lens[1] == 0
    pools = [c for c in GPU.E2E_CASES if c["bags"]]
    assert {routes[c["name"]]["pool"] for c in pools} == {DR.POOL_GATHER_VEC4, DR.POOL_GATHER_SCALAR} and any(c["psw"] for c in pools)
    for c in pools:
        assert np.array_equal(np.diff(batches[c["name"]]["offsets"]), lens)
    # pool_gather4_kernel's spans
    for c in (x for x in GPU.E2E_CASES if x["span"]):
        b = batches[c["name"]]
        N = b["N"]
        assert N == c["span"] and routes[c["name"]]["pool"] == (DR.POOL_SPAN if N > DR.POOL_SPAN_MIN else DR.POOL_GATHER_VEC4)
        starts = b["offsets"][:-1][np.diff(b["offsets"]) > 0]
        head = np.zeros(N, dtype=bool)
        head[starts] = True
        assert head[:64].all(), "a span of 64 one-lookup bags"
        assert head[64] and not head[65:264].any() and not head[128:192].any(), "a bag from lane 0; a span with no head"
        assert head[319] and 319 % 64 == 63 and not head[320:401].any() and head[401], "a bag from lane 63 running 81 lookups on"
        assert (np.diff(b["offsets"]) == 0).any() and b["offsets"][-1] == N
    assert {c["span"] for c in GPU.E2E_CASES if c["span"]} == {DR.POOL_SPAN_MIN, DR.POOL_SPAN_MIN + 1}
    assert (DR.POOL_SPAN_MIN + 1) % 64 == 1, "the last span of 65,537 lookups is partial"
