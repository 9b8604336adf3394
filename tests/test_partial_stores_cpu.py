"""No GPU needed: the benchmark shape's backward stores its partial gradients as whole float4s (csrc/ttx_tt_spec.inc, Shape3::W16).

Read off the gfx950 listing of the rank-32 translation unit -- the one tests/test_kernel_resources.py builds, reused when it is
newer than the sources -- through scripts/asm_stats.py: the non-padded single-sub-chunk Shape3<32,4,32,4,...> instantiations of
spec_bwd_kernel (q0 = 4 and q0 = 2) hold no non-temporal and no write-through 32-bit vector store to
global memory, and exactly four plain ones, none of which stores a result: work-group 0's reset of reduce_apply's arrival
counters (zero_hot_counters) and the markers of the three ablation exits (`dbg & 16`, `& 32`, `& 64`: one float to pc[0][0] under
a condition that never holds, to keep the loads in front of the exit alive).  Every partial-gradient store of these kernels was
non-temporal before, so a 4-byte store of a partial would show as a non-temporal one, or as a fifth plain one.  A
write-through store narrower than 16 bytes costs about six times per byte, which is why the flavour can be chosen per launch only
once every partial store is a float4.

The sub-chunk walk (MULTI, batches of 131072 lookups and more) keeps its 4-byte non-temporal stores: its launches hand over more
than the Infinity Cache holds, so write-through has nothing to offer there, and the 16-byte layout alone measured 0.2 % slower at
cfg5shard (profiles/partial_stores.md) -- those instantiations are asserted to be what they were: no write-through store."""
import glob
import os
import subprocess
import sys

import pytest

from test_kernel_resources import CSRC, HIPCC, PRELOAD, ROOT


@pytest.fixture(scope="module")
def spec32_listing():
    asm = os.path.join(ROOT, "build", "asm", "spec32_test.s")
    srcs = [f for ext in ("*.hip", "*.h", "*.inc") for f in glob.glob(os.path.join(CSRC, ext))]
    if not os.path.exists(asm) or any(os.path.getmtime(f) > os.path.getmtime(asm) for f in srcs):
        os.makedirs(os.path.dirname(asm), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed", *PRELOAD,
                        "-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "ttx_tt_spec32.hip")], check=True, timeout=900,
                       capture_output=True)
    return asm


def test_benchmark_shape_backward_stores_no_partial_as_dwords(spec32_listing):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import asm_stats

    seen = walk = 0
    for name, stores in asm_stats.vmem_stores(spec32_listing).items():
        # <32,4,32,4, passes, chunk, q0>, then <MULTI, PAD = false>
        if "spec_bwd_kernel" not in name or "Shape3ILi32ELi4ELi32ELi4E" not in name or "ELb0EEEv" not in name:
            continue
        assert stores, name
        assert all(bits in (32, 64, 96, 128) for bits, _, _ in stores), (name, stores)
        if "EEELb1ELb0EEEv" in name:  # the sub-chunk walk: as it was
            assert not any("sc1" in mods for _, mods, _ in stores), (name, stores)
            walk += 1
            continue
        narrow = [mods for bits, mods, _ in stores if bits == 32]
        assert not [m for m in narrow if m], (name, narrow)   # no nt / sc0 / sc1 dword store
        assert len(narrow) == 4, (name, len(narrow))          # the counter reset and the three ablation markers
        wide = [mods for bits, mods, results in stores if bits == 128 and results]
        # both flavours of the three store sites are there: non-temporal and write-through
        assert any("nt" in m for m in wide) and any("sc1" in m for m in wide), (name, wide)
        seen += 1
    assert seen == 2 and walk == 2, (seen, walk)  # q0 = 4 and q0 = 2
