"""tests/golden/hashref_values.npz: what the REFERENCE's own hash functions (oracle/_ref/libhashref.so, compiled from its
hashtbl_cuda_utils.cuh by oracle/Makefile) return for the keys and table sizes of tests/test_oracle_golden.py::
test_hash_vs_reference_build -- the test compares the oracle with these where that build is absent.
Run from the repository root after build(), where the reference tree lies:  python tests/golden/make_hashref_values.py"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_oracle_golden import hashref_cases  # noqa: E402

keys, sizes, keys32, size32 = hashref_cases()
ref = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libhashref.so"))
ref.ref_hash64.restype = C.c_uint32
ref.ref_hash64.argtypes = [C.c_int64, C.c_int32]
ref.ref_hash32.restype = C.c_uint32
ref.ref_hash32.argtypes = [C.c_int32, C.c_int32]
h64 = np.array([[ref.ref_hash64(int(k), s) for k in keys] for s in sizes], dtype=np.uint32)
h32 = np.array([ref.ref_hash32(int(k), size32) for k in keys32], dtype=np.uint32)
np.savez_compressed(os.path.join(HERE, "hashref_values.npz"), keys=keys, sizes=np.array(sizes, dtype=np.int64), hash64=h64,
                    keys32=keys32, hash32=h32)
print("hashref_values.npz:", h64.shape, h32.shape)
