"""Host reference of kmx_count_unitig_clean, written straight from the rule in include/kmx.h on top of tests/link_np.py: one loop over
the unitigs that states the three reasons, Python ints for the products of the order LOSES.  Nothing here knows about lanes, limbs
or the order in which a kernel would look things up.  Shared by tests/test_gpu_unitig_clean.py; pinned against expectations built
from strings alone in tests/test_clean_np.py, which needs no GPU.

An oriented unitig is t = 2 * u + s; mirror(t) = t ^ 1.  `rule` everywhere is a dict of the call's six integer parameters."""
import numpy as np

from tests import link_np

CLEAN_KEEP, CLEAN_TIP, CLEAN_BUBBLE, CLEAN_ISLAND = 0, 1, 2, 3
RULE_NAMES = ("tip_max_nodes", "tip_num", "tip_den", "bubble_max_nodes", "bubble_max_diff", "island_max_nodes")


def rule_of(k, tip_max_nodes=None, tip_ratio=(1, 1), bubble_max_nodes=None, bubble_max_diff=4, island_max_nodes=0):
    """the Python layer's arguments and defaults -> the six integers of the C call"""
    num, den = (0, 1) if tip_ratio is None else tip_ratio
    return dict(tip_max_nodes=k if tip_max_nodes is None else tip_max_nodes, tip_num=num, tip_den=den,
                bubble_max_nodes=2 * k if bubble_max_nodes is None else bubble_max_nodes, bubble_max_diff=bubble_max_diff,
                island_max_nodes=island_max_nodes)


def loses(s_u, m_u, u, s_y, m_y, y, a, b):
    """u LOSES to y at (a, b): the mean count per node of u is below a / b of y's, ties to the smaller index"""
    left, right = s_u * m_y * b, s_y * m_u * a
    return left < right or (left == right and u > y)


def clean_np(offsets, circular, sums, link_offsets, targets, tip_max_nodes, tip_num, tip_den, bubble_max_nodes, bubble_max_diff,
             island_max_nodes):
    """-> (keep uint8[U], reason uint8[U]); circular and sums may be None"""
    offs = [int(x) for x in np.asarray(offsets, np.uint64)]
    lo = [int(x) for x in np.asarray(link_offsets, np.uint64)]
    tg = [int(x) for x in np.asarray(targets, np.uint64)]
    U, n_links = len(offs) - 1, len(tg)
    circ = [0] * U if circular is None else [int(x) for x in circular]

    def m(u):
        return offs[u + 1] - offs[u] if offs[u + 1] >= offs[u] else 0

    def S(u):
        return m(u) if sums is None else int(np.uint64(sums[u]))

    def L(t):
        a, b = lo[t], lo[t + 1]
        if not (a <= b <= n_links and b - a <= 4):
            return []
        out = tg[a:b]
        return out if all(x < 2 * U for x in out) else []

    def lose(u, y, a, b):
        return loses(S(u), m(u), u, S(y), m(y), y, a, b)

    reason = np.zeros(U, np.uint8)
    for u in range(U):
        if circ[u]:
            continue
        d0, d1 = len(L(2 * u)), len(L(2 * u + 1))
        if d0 == 0 and d1 == 0:
            if island_max_nodes > 0 and m(u) <= island_max_nodes:
                reason[u] = CLEAN_ISLAND
        elif d0 == 0 or d1 == 0:
            if tip_max_nodes > 0 and m(u) <= tip_max_nodes:
                t = 2 * u if d0 else 2 * u + 1
                if tip_num == 0 or any(z >> 1 != u and lose(u, z >> 1, tip_num, tip_den) for x in L(t) for z in L(x ^ 1)):
                    reason[u] = CLEAN_TIP
        elif d0 == 1 and d1 == 1:
            if not (bubble_max_nodes > 0 and m(u) <= bubble_max_nodes):
                continue
            x, s = L(2 * u)[0], L(2 * u + 1)[0] ^ 1
            ls = L(s)
            if len(ls) != 2 or ls[0] == ls[1] or 2 * u not in ls:
                continue
            y = ls[0] if ls[1] == 2 * u else ls[1]
            yu = y >> 1
            lx = L(x ^ 1)
            if len(lx) != 2 or set(lx) != {2 * u ^ 1, y ^ 1}:
                continue
            if L(y) != [x] or L(y ^ 1) != [s ^ 1]:
                continue
            if u == yu or u in (s >> 1, x >> 1) or yu in (s >> 1, x >> 1):
                continue
            if circ[yu] or m(yu) > bubble_max_nodes or abs(m(u) - m(yu)) > bubble_max_diff:
                continue
            if lose(u, yu, 1, 1):
                reason[u] = CLEAN_BUBBLE
    return (reason == 0).astype(np.uint8), reason


def bubble_partner(u, link_offsets, targets):
    """the other branch of the simple bubble u was dropped from (consistent links)"""
    lo, tg = [int(x) for x in link_offsets], [int(x) for x in targets]
    s = tg[lo[2 * u + 1]] ^ 1
    (y,) = [t for t in tg[lo[s]:lo[s + 1]] if t != 2 * u]
    return y >> 1


def clean_table_np(tk, tc, k, min_count, rule):
    """one round on the host -> (keys, counts, keep, reason, (out, place, link_offsets, targets))"""
    out, place, lo, tg = link_np.links_of_table_np(tk, tc, k, min_count)
    keep, reason = clean_np(out[1], out[2], out[3], lo, tg, **rule)
    return (*link_np.select_np(tk, tc, place, out[1], keep), keep, reason, (out, place, lo, tg))


def simplify_np(tk, tc, k, min_count=1, rounds=4, **rule):
    """Context.count_simplify(2) on the host -> (keys, counts, log): rounds until one removes nothing"""
    log = []
    for _ in range(rounds):
        n = len(tc)
        if n == 0:
            break
        tk, tc, keep, reason, _ = clean_table_np(tk, tc, k, min_count, rule)
        c = np.bincount(reason, minlength=4)
        log.append({"tips": int(c[1]), "bubbles": int(c[2]), "islands": int(c[3]), "removed": n - len(tc)})
        if log[-1]["removed"] == 0:
            break
    return tk, tc, log
