"""Cases of the lineage tests that need no device to be stated: the hand-written database with every node spelled out, the
taxonomies hung over the synthetic databases, and the posting-list edges.  tests/test_lca_cases_cpu.py holds them against the
oracle; tests/test_gpu_lca.py asks the device the same questions."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_DEPTH = 16


def tree_from_paths(paths):
    """(parent uint32, depth uint8, leaf uint32) from one path per reference (a tuple of names from the top down; () = no
    lineage: the root).  A node is a path prefix; nodes are numbered by (depth, path), so parent[v] < v."""
    prefixes = {()}
    for p in paths:
        for d in range(1, len(p) + 1):
            prefixes.add(tuple(p[:d]))
    nodes = sorted(prefixes, key=lambda p: (len(p), p))
    at = {p: v for v, p in enumerate(nodes)}
    parent = np.array([at[p[:-1]] if p else 0 for p in nodes], dtype=np.uint32)
    depth = np.array([len(p) for p in nodes], dtype=np.uint8)
    leaf = np.array([at[tuple(p)] for p in paths], dtype=np.uint32).reshape(-1)
    return parent, depth, leaf


# ---- the hand-written database: six references over a depth-3 tree -------------------------------------------------------
#   node 0 root
#        1 family A          2 family B            (the two top-level clades: "kingdoms" for a hash they share)
#        3 genus A1 (in 1)   4 genus A2 (in 1)     5 genus B1 (in 2)
#        6 species A1x (in 3)   7 species A2x (in 4)   8 species B1x (in 5)
HAND_PARENT = np.array([0, 0, 0, 1, 1, 2, 3, 4, 5], dtype=np.uint32)
HAND_DEPTH = np.array([0, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.uint8)
#   reference 0, 1: two strains of species A1x   2: named at GENUS A1 only   3: species A2x   4: species B1x   5: no lineage
HAND_LEAF = np.array([6, 6, 3, 7, 8, 0], dtype=np.uint32)
HAND_REFS = [np.array(r, dtype=np.uint64) for r in
             ([10, 20, 21, 22, 25], [20, 23, 25], [11, 23, 25], [21, 24, 25], [22, 30], [12, 24])]
HAND_SAMPLE = np.array([5, 10, 11, 12, 20, 21, 22, 23, 24, 25, 27, 30, 1000], dtype=np.uint64)
HAND_ABUND = np.arange(1, 14, dtype=np.int64)
#   5: absent   10: ref 0 alone (species)   11: ref 2 alone (the genus node)   12: ref 5 alone (no lineage: root)
#   20: refs 0, 1 (inside one species)   21: refs 0, 3 (two genera of family A)   22: refs 0, 4 (two kingdoms: root)
#   23: refs 1, 2 (a species and the genus above it: the genus)   24: refs 3, 5 (a holder without a lineage: root)
#   25: refs 0, 1, 2, 3 (family A)   27: absent   30: ref 4 alone   1000: above the database's largest hash
HAND_NODES = np.array([NONE, 6, 3, 0, 6, 1, 0, 3, 0, 1, NONE, 8, NONE], dtype=np.uint32)
HAND_COUNTS = np.array([[3, 4 + 7 + 9], [2, 6 + 10], [0, 0], [2, 3 + 8], [0, 0], [0, 0], [2, 2 + 5], [0, 0], [1, 12]], dtype=np.uint64)


def pack(refs):
    offsets = np.zeros(len(refs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
    return np.concatenate(refs).astype(np.uint64), offsets


# ---- a taxonomy over clusters of five members plus independent references ------------------------------------------------
def cluster_paths(cluster_of, member_of):
    """One path per reference.  cluster_of[j] < 0: an independent reference, a species of its own in one of seven families.
    Otherwise member_of[j] in 0..4 of cluster c, spread so that the hashes the members share resolve at every depth:
      c % 3 == 0: members 0, 1 one species; 2 another species of the genus; 3 another genus of the family; 4 another family
      c % 3 == 1: one genus: members 0, 4 one species, 2 and 3 species of their own, member 1 named at the GENUS itself
      c % 3 == 2: members 1, 2 one species in a second genus; member 3 has no lineage; member 4 is named at the FAMILY"""
    paths = []
    for j, (c, k) in enumerate(zip(cluster_of, member_of)):
        c, k = int(c), int(k)
        if c < 0:
            paths.append((f"I{j % 7}", f"I{j % 7}g{j}", f"I{j % 7}g{j}s"))
            continue
        f, g0, g1 = f"F{c}", f"F{c}g0", f"F{c}g1"
        table = (
            ((f, g0, g0 + "s0"), (f, g0, g0 + "s0"), (f, g0, g0 + "s1"), (f, g1, g1 + "s0"), (f"X{c}", f"X{c}g", f"X{c}gs")),
            ((f, g0, g0 + "s0"), (f, g0), (f, g0, g0 + "s1"), (f, g0, g0 + "s2"), (f, g0, g0 + "s0")),
            ((f, g0, g0 + "s0"), (f, g1, g1 + "s0"), (f, g1, g1 + "s0"), (), (f,)),
        )[c % 3]
        paths.append(table[k])
    return paths


# ---- posting lists of chosen lengths whose answer is a species, a family and the root in turn --------------------------
EDGE_LENGTHS = (2, 3, 4, 5, 63, 64, 65, 300)
EDGE_REFS = 600  # 0..299 species S0 of genus G0 of family F0; 300..449 species S1 of genus G1 of F0; 450..599 species S2 of family F1


def edge_database(rng, max_hash, private=40):
    """(refs, parent, depth, leaf, cases): for every length L of EDGE_LENGTHS three pairs of hashes held by exactly L
    references -- references 0..L-1 (one species); 0..L-2 and 300 (another genus of the family: the LAST holder of the list
    lifts the fold); 0..L-2 and 450 (another family: the root) -- plus `private` hashes per reference.  cases: (hash, L,
    expected node)."""
    paths = [("F0", "G0", "S0")] * 300 + [("F0", "G1", "S1")] * 150 + [("F1", "G2", "S2")] * 150
    parent, depth, leaf = tree_from_paths(paths)
    species, family = int(leaf[0]), int(parent[parent[leaf[0]]])
    pool = np.unique(rng.integers(1, max_hash, size=EDGE_REFS * private + 1000, dtype=np.uint64))
    rng.shuffle(pool)
    held = [[] for _ in range(EDGE_REFS)]
    cases, at = [], 0
    for L in EDGE_LENGTHS:
        for last, want in ((L - 1, species), (300, family), (450, 0)):
            for _ in range(2):
                h = pool[at]
                at += 1
                for j in list(range(L - 1)) + [last]:
                    held[j].append(h)
                cases.append((int(h), L, want))
    for j in range(EDGE_REFS):
        held[j].extend(pool[at:at + private])
        at += private
    refs = [np.unique(np.array(h, dtype=np.uint64)) for h in held]
    return refs, parent, depth, leaf, cases


def chain_tree(n_refs):
    """A chain of depth exactly MAX_DEPTH (node v's parent is v - 1) with reference j hung at node j % (MAX_DEPTH + 1): the LCA
    of a set of holders is the SHALLOWEST of their nodes, and the deepest pair is lifted MAX_DEPTH times."""
    parent = np.array([0] + list(range(MAX_DEPTH)), dtype=np.uint32)
    depth = np.arange(MAX_DEPTH + 1, dtype=np.uint8)
    leaf = (np.arange(n_refs) % (MAX_DEPTH + 1)).astype(np.uint32)
    return parent, depth, leaf
