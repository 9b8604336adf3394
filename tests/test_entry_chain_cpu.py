"""The entry chain of the single-sub-chunk contraction kernels at the benchmark shape, from the compiler's listing (hipcc
cross-compiles gfx950 without a GPU), and the host's magic pair for the table of a pivot slice.

At the benchmark batch every work-group of a launch walks the same chain at the same time -- arguments -> chunk record ->
lookup records -> operands -> first MFMA -- and nothing else runs on the chip meanwhile.  profiles/entry_chain.md: the listing
held more trips than those.  Scalar loads of single arguments (the debug mask, then B / p_1) stood one behind the other
between the chunk record and the lookup records' requests, with the ~30 instructions of `s / p_1` behind them, and the first
core_1 block of the backward was requested behind the wait for the records, in the operand round.  Guarded here, for
spec_fwd_kernel and spec_bwd_kernel<Shape3<32,4,32,4,2,16,4>, MULTI = false, PAD = false>:
  * between the wait for the chunk record and the first lookup-record load there is no scalar load and no v_rcp (a division);
  * at least two 16-byte loads of the core_1 block stand between the chunk record's wait and the wait that follows the record
    loads, on the path of a plan that carries bag rows;
  * neither kernel uses scratch;
and table_div / table_quot (csrc/ttx_magic.h) against s / p_1 over whole ranges, in a stand-alone program."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]  # as __graft_entry__.build() compiles the product
SMALL = "Shape3ILi32ELi4ELi32ELi4ELi2ELi16ELi4EEELb0"    # (.., passes 2, chunk 16, q0 4), one sub-chunk
KERNELS = (("spec_bwd_kernel", SMALL + "ELb0E"), ("spec_fwd_kernel", SMALL + "ELb0ELb0E"))


@pytest.fixture(scope="module")
def listing():
    """(assembly listing, compiler's resource report) of the rank-32 translation unit, one compilation"""
    out = os.path.join(ROOT, "build", "asm")
    os.makedirs(out, exist_ok=True)
    asm, res = os.path.join(out, "spec32_entry_test.s"), os.path.join(out, "spec32_entry_test.res")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed", *PRELOAD,
                        "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", asm,
                        os.path.join(CSRC, "ttx_tt_spec32.hip")], check=True, timeout=900, capture_output=True, text=True)
    with open(res, "w") as f:
        f.write(r.stderr)
    return asm, res


def kernel_lines(asm_path, *needles):
    """instruction lines AND block labels of the one kernel whose mangled name holds every needle"""
    text = open(asm_path).read()
    names = [n for n in re.findall(r"^(_Z\w+):", text, re.M) if all(x in n for x in needles)]
    assert len(names) == 1, (needles, len(names))
    beg = text.index("\n" + names[0] + ":")
    end = text.index(".Lfunc_end", beg)
    out = []
    for ln in text[beg:end].splitlines()[2:]:
        ln = ln.split(";")[0].strip()
        if ln and (re.match(r"^\.LBB\d+_\d+:$", ln) or not ln.startswith(".")):
            out.append(ln)
    return names[0], out


def entry_chain(body):
    """-> (i_chunk, i_wait, i_rec, path): the chunk record's load (its address is the first pointer that arrives with the wave,
    s[2:3]), the wait for it, the first lookup-record load (an int4 without .w), and the instructions from there to the first wait
    for vector memory ON THE PATH OF A PLAN WITH BAG ROWS: that path fetches the bag row with one more dword load and then
    branches over the block that takes it from rowidx[] (which waits for the record by itself)"""
    head = body[: next(i for i, x in enumerate(body) if x.startswith("v_mfma"))]
    # (a 16-byte load through s[2:3] with the work-group's offset in a register, or through the sum chunk_rec + 16 * blockIdx,
    #  whose low word is `s_add_u32 sA, s2, ..`)
    bases, chunk = {"s[2:3]"}, None
    for i, x in enumerate(head):
        m = re.match(r"s_add_u32 s(\d+), s2, s\d+$", x)
        if m:
            bases.add(f"s[{m.group(1)}:{int(m.group(1)) + 1}]")
        m = re.match(r"(?:s_load_dwordx4 s\[\d+:\d+\]|global_load_dwordx4 v\[\d+:\d+\], v\d+), (s\[\d+:\d+\])", x)
        if m and m.group(1) in bases:
            chunk = i
            break
    assert chunk is not None, "no 16-byte load of the chunk record in front of the first MFMA"
    cnt = "lgkmcnt" if head[chunk].startswith("s_load") else "vmcnt"
    wait = next(i for i in range(chunk + 1, len(head)) if head[i].startswith("s_waitcnt") and cnt in head[i])
    rec = next(i for i in range(wait + 1, len(head)) if head[i].startswith("global_load_dwordx3"))
    path, i, row_load, jumped = [], rec + 1, False, False
    while i < len(head):
        ln = head[i]
        m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)$", ln)
        if m and row_load and not jumped and m.group(1) + ":" in head[i:]:
            i, jumped = head.index(m.group(1) + ":", i), True
            continue
        row_load |= ln.startswith("global_load_dword ")
        path.append(ln)
        if ln.startswith("s_waitcnt") and "vmcnt" in ln:
            break
        i += 1
    assert path and path[-1].startswith("s_waitcnt"), "no wait for the lookup records in front of the first MFMA"
    return chunk, wait, rec, path, head


@pytest.mark.parametrize("kern,flags", KERNELS, ids=[k for k, _ in KERNELS])
def test_no_argument_trip_and_no_division_behind_the_chunk_record(listing, kern, flags):
    name, body = kernel_lines(listing[0], kern, flags)
    chunk, wait, rec, path, head = entry_chain(body)
    between = [x for x in head[wait + 1:rec] if not x.endswith(":")]
    smem = [x for x in between if x.startswith(("s_load", "s_buffer_load"))]
    assert not smem, f"{kern}: scalar loads between the chunk record's wait and the lookup records' request: {smem}"
    rcp = [x for x in between if x.startswith("v_rcp")]
    assert not rcp, f"{kern}: a division between the chunk record's wait and the lookup records' request: {rcp}"
    # ... and none in FRONT of its request either: behind the preload header (it ends with the first s_branch) nothing waits
    # before the chunk record is asked for -- the arguments travel with it
    start = next((i for i, x in enumerate(head[:chunk]) if x.startswith("s_branch")), 0)
    early = [x for x in head[start:chunk] if x.startswith("s_waitcnt")]
    assert not early, f"{kern}: waits in front of the chunk record's request: {early}"


@pytest.mark.parametrize("kern,flags", KERNELS, ids=[k for k, _ in KERNELS])
def test_core1_block_is_requested_with_the_lookup_records(listing, kern, flags):
    name, body = kernel_lines(listing[0], kern, flags)
    chunk, wait, rec, path, head = entry_chain(body)
    round_ = [x for x in head[wait + 1:rec] + path if x.startswith("global_load_dwordx4")]
    assert len(round_) >= 2, f"{kern}: {len(round_)} 16-byte loads in front of the wait for the lookup records ({path[-1]})"
    if kern == "spec_bwd_kernel":
        # ... and that wait leaves them in flight: it counts down to the loads issued behind the records, not to zero
        m = re.search(r"vmcnt\((\d+)\)", path[-1])
        assert m and int(m.group(1)) >= 2, path[-1]


def test_single_sub_chunk_kernels_use_no_scratch(listing):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import asm_stats

    counts, res = asm_stats.parse_asm(listing[0]), asm_stats.parse_res(listing[1])
    for kern, flags in KERNELS:
        rs = [v for k, v in res.items() if kern in k and flags in k]
        cs = [v for k, v in counts.items() if kern in k and flags in k and v.get("total")]
        assert len(rs) == 1 and len(cs) == 1, (kern, len(rs), len(cs))
        assert rs[0]["ScratchSize"] == 0 and rs[0]["VGPRs Spill"] == 0, (kern, rs[0])
        assert cs[0].get("scratch", 0) == 0, (kern, cs[0])
        if kern == "spec_bwd_kernel":
            assert rs[0]["VGPRs"] <= 104, rs[0]  # (tests/test_kernel_resources.py: four work-groups per CU and room to spare)


MAGIC_MAIN = r"""
#include "ttx_magic.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  long long bad = 0, n = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    const unsigned d = (unsigned)atol(argv[a]), T = (unsigned)atol(argv[a + 1]);
    const ttx::TableDiv t = ttx::table_div(d, (unsigned long long)T * d);
    for (unsigned long long s = 0; s < (unsigned long long)T * d; ++s, ++n)
      if (ttx::table_quot((unsigned)s, t.mul, t.sh) != (unsigned)(s / d)) ++bad;
    printf("%u %u %u %d\n", d, T, t.mul, t.sh);
  }
  printf("checked %lld bad %lld\n", n, bad);
  return bad != 0;
}
"""
P1S, TABLES = (1, 3, 58, 220, 3317), (1, 3, 26)


def test_magic_pair_is_the_quotient_over_the_whole_range(tmp_path):
    """every s in [0, tables * p_1) for p_1 in {1, 3, 58, 220, 3317} and 1, 3 and 26 tables (and one pair that needs a shift),
    through the header the kernels and the host include; with ONE table the pair is (0, 31): the quotient is 0 whatever s"""
    src, exe = tmp_path / "magic_main.cpp", tmp_path / "magic_main"
    src.write_text(MAGIC_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True, timeout=300)
    args = [str(x) for p1 in P1S for t in TABLES for x in (p1, t)] + ["1000003", "2147"]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
    lines = r.stdout.split("\n")
    want = sum(p1 * t for p1 in P1S for t in TABLES) + 1000003 * 2147
    assert f"checked {want} bad 0" in lines, lines[-3:]
    pairs = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in (ln.split() for ln in lines if re.match(r"^\d+ \d+ \d+ -?\d+$", ln))}
    assert len(pairs) == len(P1S) * len(TABLES) + 1
    for p1 in P1S:
        assert pairs[(p1, 1)] == (0, 31), (p1, pairs[(p1, 1)])
    assert pairs[(1000003, 2147)][1] > 0, pairs[(1000003, 2147)]
