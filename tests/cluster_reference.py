"""The isoenergetic cluster move (sga_cluster_move_pairs / sga_cluster_move_ladders, csrc/cluster_moves.hip) in plain numpy
and Python: the move is a function of the two configurations, the graph and one drawn integer, so a breadth-first search
is an exact reference for it.  Shared by tests/test_cluster_moves_host.py and tests/test_cluster_moves_gpu.py."""
from collections import deque

import numpy as np

import oracle

DOMAIN_CLUSTER = 5  # DOMAIN_EXCHANGE | (1 << 2): the domain word of the move's one draw


def component(rowptr, colidx, val, s_a, s_b, k):
    """Sorted sites of the connected component of {i: s_a[i] != s_b[i]} around the k-th differing site (index order),
    connected through the stored entries whose value is not zero.  No differing site: an empty array."""
    s_a, s_b = np.asarray(s_a), np.asarray(s_b)
    differ = s_a != s_b
    sites = np.nonzero(differ)[0]
    if sites.size == 0:
        return np.zeros(0, np.int64)
    seed = int(sites[int(k)])
    seen = {seed}
    queue = deque([seed])
    while queue:
        i = queue.popleft()
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            j = int(colidx[e])
            if val[e] != 0 and j != i and differ[j] and j not in seen:
                seen.add(j)
                queue.append(j)
    return np.asarray(sorted(seen), np.int64)


def levels(rowptr, colidx, val, s_a, s_b, k):
    """Breadth-first levels the search around the k-th differing site runs: the largest distance from it, plus one."""
    s_a, s_b = np.asarray(s_a), np.asarray(s_b)
    differ = s_a != s_b
    sites = np.nonzero(differ)[0]
    if sites.size == 0:
        return 0
    dist = {int(sites[int(k)]): 0}
    queue = deque(dist)
    while queue:
        i = queue.popleft()
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            j = int(colidx[e])
            if val[e] != 0 and j != i and differ[j] and j not in dist:
                dist[j] = dist[i] + 1
                queue.append(j)
    return max(dist.values()) + 1


def seed_index(seed, round_, gid, count):
    """Which of `count` differing sites the move between two replicas starts from: gid = the smaller GLOBAL id of the two."""
    w = oracle.philox([0, int(round_) & 0xFFFFFFFF, int(gid) & 0xFFFFFFFF, DOMAIN_CLUSTER],
                      [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF])[0]
    return (int(w) * int(count)) >> 32


def move(rowptr, colidx, val, s_a, s_b, seed, round_, gid):
    """(new s_a, new s_b, flipped sites) of one move."""
    s_a, s_b = np.array(s_a, np.int8), np.array(s_b, np.int8)
    count = int(np.count_nonzero(s_a != s_b))
    if count == 0:
        return s_a, s_b, np.zeros(0, np.int64)
    comp = component(rowptr, colidx, val, s_a, s_b, seed_index(seed, round_, gid, count))
    s_a[comp] = -s_a[comp]
    s_b[comp] = -s_b[comp]
    return s_a, s_b, comp


def cluster_lds_bytes(n):
    """sga_replicas.h, cluster_lds_bytes: four bitmaps of ceil(n / 32) words and 64 bytes beside them."""
    return 16 * ((n + 31) // 32) + 64
