"""numpy restatement of ttx_cache_carry (include/ttx.h, "cache refresh"): what a re-populate with
keep_trained=True leaves in cache_weight and in the cache rows' optimizer state.  Per hash slot s, with k = hashtbl[s],
n = cache_state[s] (as the populate left it) and m = old_state[s] (as it was before): the slot takes part iff k != -1,
0 <= n < cache_size and s is the slot the library's probe finds k in; a participant with 0 <= m < cache_size (kept) copies
old row m and its state to row n, any other participant (admitted) leaves row n alone and zeroes its state; rows that no
participant owns are not written."""
import numpy as np

import oracle_lib as O


def participants(hashtbl, old_state, cache_state, cache_size):
    """-> [(slot, new row, old row or -1)] of the slots that take part, in slot order"""
    hashtbl = np.ascontiguousarray(hashtbl, dtype=np.int64)
    out = []
    for s in np.nonzero((hashtbl != -1) & (cache_state >= 0) & (cache_state < cache_size))[0]:
        if O.hashtbl_find(int(hashtbl[s]), hashtbl, max_probes=3) != int(s):
            continue  # a second copy of its key: the findable copy owns the key's row
        m = int(old_state[s])
        out.append((int(s), int(cache_state[s]), m if 0 <= m < cache_size else -1))
    return out


def carry_ref(hashtbl, old_state, cache_state, old_weight, cache_weight, old_opt_state=None, opt_state=None):
    """-> (cache_weight, opt_state or None) after the carry, as new arrays; the state is [cache_size] or [cache_size, D]"""
    cache_size = cache_weight.shape[0]
    w = np.array(cache_weight, copy=True)
    st = None if opt_state is None else np.array(opt_state, copy=True)
    for _, n, m in participants(hashtbl, old_state, cache_state, cache_size):
        if m >= 0:
            w[n] = old_weight[m]
            if st is not None:
                st[n] = old_opt_state[m]
        elif st is not None:
            st[n] = 0
    return w, st
