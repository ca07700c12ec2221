"""Blocks of samples for the batched lineage pass (RefDB.lca_batch / yh_lca_batch_device), stated without a device: the
databases and trees of tests/lca_cases.py, and per case the samples of one block with their abundances.
tests/test_lca_batch_cases_cpu.py holds them against the oracle (they still hold what they are named for);
tests/test_gpu_lca_batch.py asks the device the same questions."""
from collections import namedtuple

import lca_cases as cases
import numpy as np

from yacht_amd import _lib, synth

T = _lib.YH_LCA_BATCH_TILE  # consecutive hashes of one sample a lookup workgroup takes
TABLE_SLOTS = 512  # slots of the lookup's hit table in LDS (yh_lca.hip: LB_TBITS = 9)
NARROW = 2 ** 22  # the "scaled" of tests/test_gpu_lca.py's databases: a hash range of 2^42
RETENTIONS = (1, 0.9, 0.5, 0.25, 0.1)
U32_MAX = 2 ** 32 - 1

# name; the database's CSR; the taxonomy (parent, depth, leaf); the block's samples; per sample its abundances or None
Case = namedtuple("Case", "name values offsets tree samples abunds")


def cluster_database(seed=701):
    """Eight clusters of five members and forty independent references over lca_cases.cluster_paths: shared hashes that
    resolve at every depth.  Returns (refs, values, offsets, tree)."""
    rng = np.random.default_rng(seed)
    refs = synth.independent_refs(rng, 40, 1000, 0.3, 300, 3000, scaled=NARROW) + synth.clustered_refs(rng, 8, RETENTIONS, 1500, scaled=NARROW)
    values, offsets = synth.pack(refs)
    cluster_of = np.array([-1] * 40 + [c for c in range(8) for _ in RETENTIONS])
    member_of = np.array([0] * 40 + [k for _ in range(8) for k in range(len(RETENTIONS))])
    return refs, values, offsets, cases.tree_from_paths(cases.cluster_paths(cluster_of, member_of))


def draw(rng, values, n, max_hash):
    """A strictly ascending sample of exactly n hashes: about half of them hashes of the database, the rest noise."""
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    distinct, held = np.unique(values, return_counts=True)
    n_known = min((n + 1) // 2, distinct.size)
    shared = distinct[held >= 2]  # (half of the known hashes from the shared ones, as far as there are any)
    known = rng.choice(shared, size=min(n_known // 2, shared.size), replace=False)
    known = np.union1d(known, rng.choice(np.setdiff1d(distinct, known), size=n_known - known.size, replace=False))
    noise = np.setdiff1d(synth.random_sketch(rng, 2 * n + 16, max_hash), distinct)
    keep = np.union1d(known, rng.choice(noise, size=n - n_known, replace=False)).astype(np.uint64)
    assert keep.size == n
    return keep


def _abunds(rng, samples, flat=()):
    """Abundances in 1..1000 for every sample but those whose index is in `flat` (None: their hashes count once)."""
    return [None if s in flat else rng.integers(1, 1001, smp.size).astype(np.uint32) for s, smp in enumerate(samples)]


def build_cases():
    """Every block, in a fixed order, from fixed seeds."""
    out = []
    mh = synth.max_hash_for_scaled(NARROW)
    refs, values, offsets, tree = cluster_database()
    rng = np.random.default_rng(702)

    def block(name, lengths, flat=(), none=False):
        samples = [draw(rng, values, n, mh) for n in lengths]
        out.append(Case(name, values, offsets, tree, samples, None if none else _abunds(rng, samples, flat)))

    # the tile's edges, with an empty sample first, in the middle and last
    block("tile_edges", [0, 1, T - 1, T, 0, T + 1, 2 * T + 1, 0], flat=(3,))
    block("one_sample", [3 * T + 5])
    block("two_samples", [T + 7, 130])
    block("two_samples_without_abundances", [2 * T, 77], none=True)
    block("full_block", [int(n) for n in rng.integers(20, 61, 256)], flat=tuple(range(0, 256, 3)))
    # a sample wholly above the database's largest hash, one without a single hit, and one with hits between them
    top = int(values.max())
    above = np.unique(rng.integers(top + 1, top + 2 ** 30, 700, dtype=np.uint64))
    miss = np.setdiff1d(synth.random_sketch(rng, 1500, top), values)
    hit = draw(rng, values, 900, mh)
    samples = [above, hit, miss]
    out.append(Case("above_and_missing", values, offsets, tree, samples, _abunds(rng, samples)))
    # one tile whose hits land on more nodes than the hit table has slots
    rng = np.random.default_rng(703)
    n_species = 3 * TABLE_SLOTS
    pool = synth.random_sketch(rng, n_species * 4, mh)
    rng.shuffle(pool)
    crowd_refs = [np.sort(pool[j::n_species]) for j in range(n_species)]
    cv, co = synth.pack(crowd_refs)
    crowd_tree = cases.tree_from_paths([(f"F{j % 5}", f"G{j % 64}", f"S{j}") for j in range(n_species)])
    samples = [np.sort(pool)[:T + 300], np.sort(pool)[5::7]]
    out.append(Case("crowded_table", cv, co, crowd_tree, samples, _abunds(rng, samples)))
    # abundances of 2^32 - 1 on one node until its sum passes 2^32: the hand-written database, whose nodes are spelled out
    hv, ho = cases.pack(cases.HAND_REFS)
    hand_tree = (cases.HAND_PARENT, cases.HAND_DEPTH, cases.HAND_LEAF)
    samples = [cases.HAND_SAMPLE, cases.HAND_SAMPLE[:5], np.zeros(0, np.uint64), cases.HAND_SAMPLE[3:]]
    out.append(Case("hand_written", hv, ho, hand_tree, samples, [cases.HAND_ABUND.astype(np.uint32), None, None, None]))
    out.append(Case("sums_pass_32_bits", hv, ho, hand_tree, samples[:2],
                    [np.full(cases.HAND_SAMPLE.size, U32_MAX, np.uint32), np.full(5, U32_MAX, np.uint32)]))
    # the posting-list edges: lists of 2 .. 300 holders whose answer is a species, a family and the root in turn
    rng = np.random.default_rng(704)
    erefs, parent, depth, leaf, cs = cases.edge_database(rng, mh)
    ev, eo = synth.pack(erefs)
    wanted = np.array(sorted(h for h, _, _ in cs), dtype=np.uint64)
    samples = [np.union1d(wanted, np.concatenate([r[::2] for r in erefs[:80]])), wanted[::2],
               np.union1d(wanted[1::2], synth.random_sketch(rng, 2000, mh))]
    out.append(Case("posting_list_edges", ev, eo, (parent, depth, leaf), samples, _abunds(rng, samples, flat=(1,))))
    return out
