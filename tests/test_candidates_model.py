"""The model of the candidate-list searches (tests/candidates_model.py) pinned on hand-made cases on the CPU, so that the
GPU tests which compare the library with it stand on something checked:

  - the candidate set: repeats once, any input order, stale ids (below the offset, past the count, ID_NONE), deleted and
    disallowed rows, an id_offset;
  - the search form equals a brute-force numpy ranking of the set, ties between duplicate rows going to the smaller id
    even when the list names the larger id first;
  - the score form puts every score at its entry's position, the same bits at a repeated id, NaN at an ignored one."""
import numpy as np
import pytest

import candidates_model as M
from support import DT, ID_NONE, O, bits, eligible_rows, form_of, prep_of  # noqa: F401


def corpus(n=12, dim=3, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((2, dim)).astype(np.float32)


def test_candidate_set_is_sorted_distinct_and_eligible():
    el = eligible_rows(12, deleted=[4])
    assert M.candidate_rows([9, 3, 3, 7, 3, 9], 12, el).tolist() == [3, 7, 9]                  # repeats, any order
    assert M.candidate_rows([11, 10, 9, 8], 12, el).tolist() == [8, 9, 10, 11]                 # descending input
    assert M.candidate_rows([12, 13, 1 << 40, int(ID_NONE), 4, 2], 12, el).tolist() == [2]     # past the count, ID_NONE, deleted
    assert M.candidate_rows([], 12, el).size == 0
    assert M.candidate_rows([4, int(ID_NONE)], 12, el).size == 0
    # an id_offset: ids below it are no rows, the others are shifted
    assert M.candidate_rows([100, 99, 105, 111, 112, 5], 12, el, id_offset=100).tolist() == [0, 5, 11]
    # a filter: rows past the allow list are not allowed
    allow = np.zeros(6, bool)
    allow[[1, 5]] = True
    assert M.candidate_rows(range(12), 12, eligible_rows(12, allow=allow, deleted=[5])).tolist() == [1]


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
def test_search_form_is_the_ranking_of_the_set(O, metric):
    raw, rq = corpus()
    el = eligible_rows(12, deleted=[6])
    lists = [[10, 2, 2, 6, 7, 50, int(ID_NONE)], [6, 6]]
    ids, sc = M.search(O, raw, rq, 5, "f32", metric, lists, el)
    pc = O.prepare(raw, DT["f32"], prep_of(metric))
    pq = O.prepare(rq, DT["f32"], prep_of(metric))
    s = O.numpy_scores_canonical(pc[[2, 7, 10]], pq[:1], form_of(metric))[0]
    order = np.argsort(s if metric == "l2" else -s, kind="stable")
    assert ids[0].tolist() == [int(np.array([2, 7, 10])[i]) for i in order] + [int(ID_NONE)] * 2
    assert np.array_equal(bits(sc[0, :3]), bits(s[order])) and np.isnan(sc[0, 3:]).all()
    assert (ids[1] == ID_NONE).all() and np.isnan(sc[1]).all()                                 # nothing eligible in the list


def test_tie_between_duplicate_rows_goes_to_the_smaller_id(O):
    raw, rq = corpus()
    raw[9] = raw[3]                                                                            # exact duplicates
    el = eligible_rows(12)
    ids, sc = M.search(O, raw, rq[:1], 3, "f32", "cosine", [[1009, 1003, 1005]], el, id_offset=1000)   # larger id first
    ids, sc = ids[0], sc[0]
    at3, at9 = int(np.flatnonzero(ids == 1003)[0]), int(np.flatnonzero(ids == 1009)[0])
    assert at9 == at3 + 1 and bits(sc)[at3] == bits(sc)[at9]


def test_score_form_keeps_the_callers_positions(O):
    raw, rq = corpus()
    el = eligible_rows(12, deleted=[6])
    lists = [[110, 102, 102, 106, 99, 112, int(ID_NONE), 110], []]
    sc = M.score(O, raw, rq, "bf16", "l2", lists, el, id_offset=100)
    assert sc.shape == (8,) and sc.dtype == np.float32
    assert np.isnan(sc).tolist() == [False, False, False, True, True, True, True, False]
    assert bits(sc)[0] == bits(sc)[7] and bits(sc)[1] == bits(sc)[2]                          # a repeat: the same bits
    pc = O.prepare(raw, DT["bf16"], prep_of("l2"))
    pq = O.prepare(rq, DT["bf16"], prep_of("l2"))
    s = O.numpy_scores_canonical(pc[[10, 2]], pq[:1], form_of("l2"))[0]
    assert np.array_equal(bits(sc[:2]), bits(s))
    ids, lims = M.flat(lists)
    assert ids.dtype == np.uint64 and ids.size == 8 and lims.dtype == np.uint32 and lims.tolist() == [0, 8, 8]
