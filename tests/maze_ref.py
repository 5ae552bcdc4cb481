"""The maze generator (include/lmaze.h lmaze_generate) restated in numpy, for the tests of it: the Philox draws of a maze,
the edge keys, Kruskal over them (the definition of the tree), the bytes and the goal; beside it a round-synchronous Boruvka
over the same keys that reports how many rounds and pointer-jump passes it needed, and a BFS over the free cells.  It imports
nothing of the package under test."""
import functools

import numpy as np

from closed_loop_ref import philox

W, B, X = ord("W"), ord("B"), ord("X")
STREAM = 0x40000000                  # last counter word of every generator draw
KEY_MASK = 0xFFFFF800                # the weight's bits a key keeps; the low 11 carry the edge index
GRIDS = (5, 6, 8, 11, 12, 16, 32, 33, 35, 64)


def rooms_per_side(G):
    return (G - 1) // 2


def log2_ceil(n):
    return int(n - 1).bit_length()


def edge_table(G):
    """Every existing edge of the room graph: k, its two rooms, its wall cell (row, column)."""
    R = rooms_per_side(G)
    out = []
    for i in range(R):
        for j in range(R):
            r = i * R + j
            if i + 1 < R:
                out.append((2 * r, r, r + R, 2 + 2 * i, 1 + 2 * j))
            if j + 1 < R:
                out.append((2 * r + 1, r, r + 1, 1 + 2 * i, 2 + 2 * j))
    return np.array(out, np.int64).reshape(-1, 5)


def draws(G, seed, m):
    """The R*R + 1 Philox calls of maze m: uint64[R*R + 1, 4] of 32-bit words; the last row is the goal's call."""
    RR = rooms_per_side(G) ** 2
    r = np.arange(RR + 1, dtype=np.uint64)
    m, seed = int(m), int(seed)
    c0 = np.full(RR + 1, m & 0xFFFFFFFF, np.uint64)
    c1 = np.full(RR + 1, (m >> 32) & 0xFFFFFFFF, np.uint64)
    c3 = np.full(RR + 1, STREAM, np.uint64)
    return np.stack(philox(c0, c1, r, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=1)


def edge_keys(G, d):
    """key(k) and the loop draw of every existing edge, in edge_table's order."""
    e = edge_table(G)
    k = e[:, 0]
    weight = d[k >> 1, k & 1].astype(np.int64)
    loop = d[k >> 1, 2 + (k & 1)].astype(np.int64)
    return (weight & KEY_MASK) | k, loop


def kruskal(G, keys):
    """The minimum spanning tree under `keys`: a bool per existing edge.  Ascending key order, union-find."""
    e = edge_table(G)
    RR = rooms_per_side(G) ** 2
    parent = list(range(RR))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    tree = np.zeros(len(e), bool)
    for idx in np.argsort(keys, kind="stable"):
        a, b = find(int(e[idx, 1])), find(int(e[idx, 2]))
        if a != b:
            parent[a] = b
            tree[idx] = True
    return tree


def boruvka(G, keys):
    """The same tree by rounds: every component takes its minimum outgoing key, hooks onto the component at the other end
    (two components that pick each other: the smaller label stays root), pointers are jumped until nothing moves, rooms are
    relabelled.  Returns (tree, rounds that hooked, most pointer-jump passes that moved something in one round)."""
    e = edge_table(G)
    RR = rooms_per_side(G) ** 2
    comp = np.arange(RR)
    tree = np.zeros(len(e), bool)
    NONE = np.int64(1) << 32
    by_key = {int(k): i for i, k in enumerate(keys)}
    rounds = most = 0
    while True:
        cu, cv = comp[e[:, 1]], comp[e[:, 2]]
        out = cu != cv
        if not out.any():
            break
        rounds += 1
        best = np.full(RR, NONE)
        np.minimum.at(best, cu[out], keys[out])
        np.minimum.at(best, cv[out], keys[out])
        parent = np.arange(RR)
        for c in np.flatnonzero(best != NONE):
            i = by_key[int(best[c])]
            tree[i] = True
            a, b = comp[e[i, 1]], comp[e[i, 2]]
            other = b if a == c else a
            parent[c] = c if (best[other] == best[c] and c < other) else other
        passes = 0
        while True:
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt
            passes += 1
        most = max(most, passes)
        comp = parent[comp]
    return tree, rounds, most


@functools.lru_cache(maxsize=None)
def _tree_of(G, seed, m):
    d = draws(G, seed, m)
    keys, loop = edge_keys(G, d)
    return kruskal(G, keys), loop, int(d[-1, 0])


def goal_room(G, goal_draw):
    RR = rooms_per_side(G) ** 2
    return (int(goal_draw) * RR) >> 32


def assemble(G, opened, gr):
    """The bytes: 'W' everywhere, 'B' on the rooms and on the wall cells of the opened edges, 'X' on room gr."""
    R = rooms_per_side(G)
    e = edge_table(G)
    lay = np.full((G, G), W, np.uint8)
    lay[1:2 * R:2, 1:2 * R:2] = B
    lay[e[opened, 3], e[opened, 4]] = B
    gx, gy = 1 + 2 * (gr // R), 1 + 2 * (gr % R)
    lay[gx, gy] = X
    return lay, (gx, gy)


def maze(G, seed, m, loops_u32=0):
    """Maze m of (G, seed): uint8[G, G] and its goal cell (x, y)."""
    tree, loop, goal_draw = _tree_of(int(G), int(seed), int(m))
    opened = tree | (loop < int(loops_u32)) if loops_u32 else tree
    return assemble(G, opened, goal_room(G, goal_draw))


def generate(G, mazes, seed, maze_base=0, loops_u32=0):
    """What lmaze_generate writes: uint8[mazes, G, G] and int32[mazes, 2]."""
    lay = np.empty((mazes, G, G), np.uint8)
    goal = np.empty((mazes, 2), np.int32)
    for p in range(mazes):
        lay[p], goal[p] = maze(G, seed, maze_base + p, loops_u32)
    return lay, goal


def connected(lay):
    """Every non-'W' cell reaches the 'X' cell over non-'W' cells (4-neighbourhood)."""
    G = lay.shape[0]
    free = lay != W
    seen = np.zeros_like(free)
    stack = [tuple(c) for c in np.argwhere(lay == X)]
    for c in stack:
        seen[c] = True
    while stack:
        x, y = stack.pop()
        for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= nx < G and 0 <= ny < G and free[nx, ny] and not seen[nx, ny]:
                seen[nx, ny] = True
                stack.append((nx, ny))
    return bool((seen == free).all())
