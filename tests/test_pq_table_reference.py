"""The synthesized count tables of tests/test_pq_accumulate.py reach what they are built for, judged by the float64 reference alone
(tests/seg_eval_common.py): osr_pq_accumulate is one workgroup of 1024 threads that strides over the rows, the predicted ids, the
(row, id) pairs and the category slots, so the large table has more than 1024 table rows, ids, pairs and slots, with matches at
their far ends; the
multi-match table has rows with several matches, in a slot whose (g, p) summation order shows in the bits."""
from collections import Counter

import numpy as np

from tests.seg_eval_common import PQ_LARGE, PQReference, pq_large_table, pq_matches, pq_multi_match_table


def test_the_large_table_passes_1024_in_every_direction():
    G, P, ncat = PQ_LARGE["G"], PQ_LARGE["P"], PQ_LARGE["ncat"]
    counts, meta, slots = pq_large_table()
    assert counts.shape == (G + 2, P + 1) == (1025, 2048) and meta.shape == (G, 4) and slots.shape == (P,) and ncat > 1024 and G * P > 1024
    assert np.count_nonzero(counts[:, 1:]) <= 4 * P  # sparse: a few non-zero rows per predicted id
    assert np.array_equal(meta[:, 2], counts[1:G + 1].sum(axis=1))  # consistent areas
    ref = PQReference(ncat)
    ref.add(counts, meta, slots)
    matches = pq_matches(counts, meta, slots, ncat)
    assert len(matches) == int(ref.counts[:, 0].sum()) and len({g for g, *_ in matches}) == len(matches)  # at most one match per row
    for s in range(ncat):  # pq_matches restates the reference: the same terms in the same order
        terms = [m[3] for m in matches if m[2] == s]
        assert sum(terms) == ref.iou[s]
    print(f"[reference] large table: tp {ref.counts[:, 0].sum()} fp {ref.counts[:, 1].sum()} fn {ref.counts[:, 2].sum()} flags {ref.flags.tolist()}; "
          f"tp of the hot slots {[int(ref.counts[s, 0]) for s in PQ_LARGE['hot']]}")
    assert any(g == G - 1 for g, *_ in matches) and any(p == P for _, p, *_ in matches) and any(s >= 1024 for *_, s, _ in matches)
    assert any(p > 1024 for _, p, *_ in matches) and any(s < 1024 for *_, s, _ in matches)
    assert int(ref.counts[:, 0].max()) >= 100  # a long ordered sum
    assert ref.counts[:, 1].sum() > 0 and ref.counts[:, 2].sum() > 0 and ref.flags[1] > 0 and ref.flags[2] > 0
    used = np.nonzero(ref.counts.sum(axis=1))[0]
    assert used.min() < 1024 <= used.max()
    # what is mixed in
    crowd, pick, slot_g = meta[:, 1] != 0, meta[:, 3] != 0, meta[:, 0]
    assert crowd.sum() >= 20 and pick.sum() >= 5 and not (pick & ~crowd).any()
    assert len(set(slot_g[crowd].tolist()) - set(slot_g[pick].tolist())) >= 5  # crowds without a crowd_pick in their slot
    assert all(Counter(slot_g[pick].tolist())[s] == 1 for s in slot_g[pick])  # the contract: one row per slot
    assert (counts[0, 1:] > 0).sum() >= 100 and (counts[G + 1, 1:] > 0).sum() >= 100  # VOID overlap, unlisted-row mass
    assert (counts[:, 1:].sum(axis=0) == 0).sum() >= 3  # empty predictions
    assert (slot_g < 0).any() and (slot_g >= ncat).any() and (slots < 0).any() and (slots >= ncat).any()
    # a crowd shields at least one prediction that VOID alone would not: crowd_pick is observable
    no_pick = meta.copy()
    no_pick[:, 3] = 0
    other = PQReference(ncat)
    other.add(counts, no_pick, slots)
    assert other.counts[:, 1].sum() > ref.counts[:, 1].sum()


def test_the_multi_match_table_has_rows_with_several_matches_and_an_observable_order():
    ncat, slot = 4, 1
    counts, meta, slots = pq_multi_match_table(ncat=ncat, slot=slot)
    G = meta.shape[0]
    assert (meta[:, 2] < counts[1:G + 1].sum(axis=1)).sum() >= 3  # inconsistent areas: smaller than the row sums
    matches = pq_matches(counts, meta, slots, ncat)
    per_row = Counter(g for g, *_ in matches)
    multi = sorted(g for g, n in per_row.items() if n >= 2)
    single = sorted(g for g, n in per_row.items() if n == 1)
    assert len(multi) >= 3 and all(m[2] == slot for m in matches)
    assert all(any(g < m for g in single) and any(g > m for g in single) for m in multi)  # ordinary matches before and after each
    for m in multi:  # a row's partners are not neighbouring ids: ids of other rows, and ids that do not match, lie in between
        ps = [p for g, p, *_ in matches if g == m]
        assert max(ps) - min(ps) >= len(ps) + 1
    ref = PQReference(ncat)
    ref.add(counts, meta, slots)
    want = ref.iou[slot]
    assert sum(m[3] for m in matches) == want and int(ref.counts[slot, 0]) == len(matches)
    reverse = [m[3] for m in reversed(matches)]
    within = [m[3] for m in sorted(matches, key=lambda m: (m[0], -m[1]))]  # the rows in order, a row's ids descending
    p_major = [m[3] for m in sorted(matches, key=lambda m: (m[1], m[0]))]
    late = [m[3] for m in matches if per_row[m[0]] == 1] + [m[3] for m in matches if per_row[m[0]] > 1]  # the full-row walks last
    for name, terms in (("reversed", reverse), ("ids descending within a row", within), ("p-major", p_major), ("multi-match rows last", late)):
        assert sorted(terms) == sorted(m[3] for m in matches)
        assert sum(terms) != want, f"the order '{name}' must give other bits"
