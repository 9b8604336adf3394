"""The pivot's DISPATCH order (csrc/ttx_plan.hip: chunk_cols / chunk_dispatch_index), numpy only.  TEST INFRASTRUCTURE.

The one-launch and the wide plan routes deal the n chunk slots (slice-major) column-major over C = 8 columns: the slots are cut
into C segments of K = n // C or K + 1 consecutive slots (the first n % C segments take the extra one), and slot start_r + k
of segment r goes to list index C k + r.  Work-groups go round-robin over the 8 XCDs, so `index % 8` is the XCD a chunk's
work-group lands on relative to the launch's first one."""
import numpy as np

COLS = 8          # kChunkCols (csrc/ttx_internal.h)
ONE_COLUMN = 1 << 17   # ttx_debug_skip bit 17: one column, the list in slot order


def dispatch_index(x, n, cols=COLS):
    """list index of the chunk(s) with slot x (int or array) of n chunks: the closed form of the device helper"""
    x = np.asarray(x, dtype=np.int64)
    K, rem = divmod(int(n), int(cols))
    head = rem * (K + 1)
    y = np.maximum(x - head, 0)
    Kd = max(K, 1)   # (K == 0: every slot lies in the head)
    return np.where(x < head, cols * (x % (K + 1)) + x // (K + 1), cols * (y % Kd) + rem + y // Kd)


def dispatch_index_by_definition(n, cols=COLS):
    """the same map for all slots [0, n), from the segments' definition: size_r = K + (r < rem), start_r = r K + min(r, rem)"""
    K, rem = divmod(int(n), int(cols))
    out = np.empty(n, dtype=np.int64)
    for r in range(cols):
        size, start = K + (1 if r < rem else 0), r * K + min(r, rem)
        out[start:start + size] = cols * np.arange(size) + r
    return out


def slot_slices(lens1, mc):
    """slice of every slot, in slot order: slice s owns ceil(len / mc) consecutive slots"""
    rows1 = -(-np.asarray(lens1, dtype=np.int64) // int(mc))
    return np.repeat(np.arange(rows1.size), rows1)


def pairs(index, slices, cols=COLS):
    """the distinct (index % cols, slice) pairs of a list: how many times the XCDs' L2s fetch a core_1 slice from the fabric"""
    return {(int(i) % cols, int(s)) for i, s in zip(index, slices)}


def full_first_index(lens1, mc):
    """the order the routes produced BEFORE the columns: all full chunks slice-major, then the partial chunks -> index per slot"""
    lens1 = np.asarray(lens1, dtype=np.int64)
    nf, np_ = lens1 // int(mc), (lens1 % int(mc) > 0).astype(np.int64)
    fbase = np.concatenate([[0], np.cumsum(nf)])
    pbase = np.concatenate([[0], np.cumsum(np_)])
    out = []
    for s in range(lens1.size):
        out += list(fbase[s] + np.arange(nf[s]))
        if np_[s]:
            out.append(fbase[-1] + pbase[s])
    return np.asarray(out, dtype=np.int64)
