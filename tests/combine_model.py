"""The model of a search by weighted examples (vrod_search_combined): plain numpy and the CPU oracle.

  operands     the optional vector through oracle.prepare (what vrod_search does to a query), then the prepared stored
               rows -- oracle.prepare of the raw corpus, which is what vrod_index_get_rows returns -- in the order given;
  combination  a loop over the operands on np.float32 arrays: acc = acc + w * x is one multiply and one add per step, each
               rounded to fp32, which numpy never fuses;
  search       the combined vector is a raw query: oracle_over prepares it again and scans the eligible rows minus the
               query's excluded set, ids mapped back.

A query here is a dict: {"vector": [dim] or None, "vw": float or None, "terms": [local rows], "weights": [...],
"exclude": [ids, any uint64]}.  Term rows are LOCAL rows (id - id_offset); excluded ids are ids, matched by value.
"""
import numpy as np

from support import DT, ID_NONE, oracle_over, prep_of


def combine(O, pc, dtype, metric, vector, vw, terms, weights):
    """pc: the prepared corpus [n, dim] fp32.  -> the combined raw query [dim] fp32."""
    acc = np.zeros(pc.shape[1], np.float32)
    ops = []
    if vector is not None:
        pv = O.prepare(np.asarray(vector, np.float32)[None, :], DT[dtype], prep_of(metric), threads=1)[0]
        ops.append((np.float32(1.0 if vw is None else vw), pv))
    ops += [(np.float32(w), pc[int(r)]) for r, w in zip(terms, weights)]
    with np.errstate(all="ignore"):
        for w, x in ops:
            prod = (w * x).astype(np.float32)        # fl(w * x[j])
            acc = (acc + prod).astype(np.float32)    # fl(acc + ...)
    return acc


def combine_scalar(O, pc, dtype, metric, vector, vw, terms, weights):
    """combine() restated one np.float32 scalar at a time: what the vectorised loop must equal bit for bit."""
    dim = pc.shape[1]
    ops = []
    if vector is not None:
        pv = O.prepare(np.asarray(vector, np.float32)[None, :], DT[dtype], prep_of(metric), threads=1)[0]
        ops.append((np.float32(1.0 if vw is None else vw), pv))
    ops += [(np.float32(w), pc[int(r)]) for r, w in zip(terms, weights)]
    out = np.empty(dim, np.float32)
    for j in range(dim):
        acc = np.float32(0.0)
        for w, x in ops:
            acc = np.float32(acc + np.float32(w * np.float32(x[j])))
        out[j] = acc
    return out


def combine_fp64(O, pc, dtype, metric, vector, vw, terms, weights):
    """The same operands accumulated in fp64 and rounded once at the end: what a fused or widened kernel would give."""
    acc = np.zeros(pc.shape[1], np.float64)
    if vector is not None:
        pv = O.prepare(np.asarray(vector, np.float32)[None, :], DT[dtype], prep_of(metric), threads=1)[0]
        acc += np.float64(np.float32(1.0 if vw is None else vw)) * pv.astype(np.float64)
    for r, w in zip(terms, weights):
        acc += np.float64(np.float32(w)) * pc[int(r)].astype(np.float64)
    return acc.astype(np.float32)


def excluded_ids(query, exclude_terms, id_offset=0):
    ex = [int(x) for x in query.get("exclude", ())]
    if exclude_terms:
        ex += [int(r) + id_offset for r in query["terms"]]
    return ex


def search(O, raw, pc, dtype, metric, queries, k, eligible, exclude_terms=False, id_offset=0):
    """raw / pc: the raw and the prepared corpus; eligible: ascending local rows a search may return.
    -> (ids uint64 [nq, k], scores float32 [nq, k])."""
    nq = len(queries)
    oi = np.full((nq, k), ID_NONE, np.uint64)
    osc = np.full((nq, k), np.nan, np.float32)
    eligible = np.asarray(eligible, np.int64)
    if not nq:
        return oi, osc
    comb = np.stack([combine(O, pc, dtype, metric, Q.get("vector"), Q.get("vw"), Q["terms"], Q["weights"]) for Q in queries])
    sets = [np.array(excluded_ids(Q, exclude_terms, id_offset), dtype=np.uint64) for Q in queries]
    plain = [q for q in range(nq) if sets[q].size == 0]          # nothing excluded: one batched oracle call serves them all
    if plain:
        oi[plain], osc[plain] = oracle_over(O, raw, np.ascontiguousarray(comb[plain]), k, dtype, metric, eligible, id_offset)
    for q in range(nq):
        if sets[q].size:
            keep = eligible[~np.isin(eligible.astype(np.uint64) + np.uint64(id_offset), sets[q])]
            oi[q], osc[q] = (a[0] for a in oracle_over(O, raw, comb[q][None, :], k, dtype, metric, keep, id_offset))
    return oi, osc


def flat(queries):
    """The queries as the C arguments: (vectors [nq, dim] or None, vector_weights [nq] or None, term_lims, term_ids (LOCAL
    rows, the caller adds id_offset), term_weights, exclude_lims, exclude_ids).  Vectors: all queries or none."""
    has_vec = [Q.get("vector") is not None for Q in queries]
    assert all(has_vec) or not any(has_vec)
    vec = np.ascontiguousarray(np.stack([Q["vector"] for Q in queries]), np.float32) if all(has_vec) and queries else None
    vw = None
    if vec is not None and any(Q.get("vw") is not None for Q in queries):
        vw = np.array([1.0 if Q.get("vw") is None else Q["vw"] for Q in queries], np.float32)
    tl = np.cumsum([0] + [len(Q["terms"]) for Q in queries]).astype(np.uint32)
    tid = np.array([r for Q in queries for r in Q["terms"]], dtype=np.uint64)
    tw = np.array([w for Q in queries for w in Q["weights"]], dtype=np.float32)
    xl = np.cumsum([0] + [len(Q.get("exclude", ())) for Q in queries]).astype(np.uint32)
    xid = np.array([x for Q in queries for x in Q.get("exclude", ())], dtype=np.uint64)
    return vec, vw, tl, tid, tw, xl, xid
