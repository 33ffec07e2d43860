"""Pure-Python restatement of include/kge_hip_filtered.h: the seven steps of kge_filtered_corrupt for one position and for
a batch in tile order, kge_triples_known, and the brute-force enumeration both are checked against."""
import bisect

MASK64 = (1 << 64) - 1


def replace(x, L, draw, n_ent):
    """(replacement, exhausted) of one position: ``x`` the entity being replaced, ``L`` the ascending distinct list of
    known answers, ``draw`` any Python int (read as its 64-bit pattern)."""
    m = len(L)
    below = bisect.bisect_left(L, x)                    # #{l in L : l < x}
    inside = below < m and L[below] == x
    c = n_ent - m - (0 if inside else 1)
    if c <= 0:
        return x, 1
    v = (draw & MASK64) % c
    if not inside:
        v += v >= x - below
    lo, hi = 0, m                                       # j = #{j : L[j] - j <= v}
    while lo < hi:
        mid = (lo + hi) // 2
        if L[mid] - mid <= v:
            lo = mid + 1
        else:
            hi = mid
    return v + lo, 0


def free_entities(x, L, n_ent):
    """Brute force: the entities that are neither in L nor x, ascending."""
    known = set(L)
    return [e for e in range(n_ent) if e not in known and e != x]


def corrupt(h, t, n_neg, mask, draws, tail_lists, head_lists, n_ent):
    """(neg_h, neg_t, exhausted) lists of B * n_neg positions in tile order; ``tail_lists[i]`` / ``head_lists[i]`` are the
    ascending lists of fact i."""
    B = len(h)
    neg_h, neg_t, ex = [], [], []
    for p in range(B * n_neg):
        i = p % B
        if mask[p]:
            e, x = replace(h[i], head_lists[i], draws[p], n_ent)
            neg_h.append(e)
            neg_t.append(t[i])
        else:
            e, x = replace(t[i], tail_lists[i], draws[p], n_ent)
            neg_h.append(h[i])
            neg_t.append(e)
        ex.append(x)
    return neg_h, neg_t, ex


def known(index, key1, key2, value):
    """``index``: {(k1, k2): set or list}; 1 where value[p] is in the list of (key1[p], key2[p]), 0 for an absent key."""
    return [int(v in index.get((a, b), ())) for a, b, v in zip(key1, key2, value)]
