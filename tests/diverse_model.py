"""The model of a diversified search (vrod_search_diverse): ModelIndex plus exact greedy MMR over the oracle's top pool.

The pool is `ModelIndex.search(rq, pool)`; g comes from oracle.numpy_scores_canonical over the pool's prepared rows (the
chain is symmetric in its operands, so which side is "the query" does not matter); the greedy loop is written in explicit
np.float32 steps: every product and the difference rounded once, nothing fused.  Rules as include/vrod.h states them:
  pen   folded in selection order; a NaN g changes nothing, a number replaces a NaN pen, otherwise only a strictly better
        g (larger for cosine / ip, smaller for l2) replaces pen;
  step  the best v over the positions not taken: NaN loses to any number, -0.0 == +0.0, ties (an all-NaN step included)
        go to the smaller position.
"""
import numpy as np

from index_model import ID_NONE, METRIC_L2, ModelIndex
from oracle import oracle as O

MAX_DIVERSE_POOL = 1024


def check_args(k, pool, lam):
    """diverse_plan.h diverse_check_args: 0 = fine."""
    if k == 0:
        return 1
    if k > pool:
        return 2
    if pool > MAX_DIVERSE_POOL:
        return 3
    if not (0.0 <= lam <= 1.0):
        return 4
    return 0


def greedy(r, G, k, lam, lower_is_better):
    """r [m] float32, G [m, m] float32 -> (positions, v at selection) of min(k, m) greedy steps."""
    m = r.shape[0]
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    pen = np.full(m, np.nan, np.float32)
    taken = np.zeros(m, bool)
    order, vals = [], []
    with np.errstate(all="ignore"):
        a = (lam * r).astype(np.float32)                             # fl(lambda * r_i): the same at every step
        for t in range(min(k, m)):
            if t == 0:
                sel, v = 0, a[0]
            else:
                b = (mu * pen).astype(np.float32)
                vs = (a - b).astype(np.float32)
                nan = np.isnan(vs)
                val = np.where(nan, np.float32(0), vs if lower_is_better else -vs) + np.float32(0)   # -0 -> +0
                o = np.lexsort((np.arange(m), val, nan, taken))      # not taken first, NaN last, the value, the position
                sel = int(o[0])
                v = vs[sel]
            taken[sel] = True
            order.append(sel)
            vals.append(v)
            g = G[sel]
            better = (g < pen) if lower_is_better else (g > pen)
            pen = np.where(~np.isnan(g) & (np.isnan(pen) | better), g, pen).astype(np.float32)
    return np.asarray(order, np.int64), np.asarray(vals, np.float32)


class DiverseModel(ModelIndex):
    def pools(self, rq, pool):
        """The part of a diversified search that k and lambda do not touch -> (ids [nq, pool], scores [nq, pool], [G per
        query]): compute it once, select from it with many (k, lambda)."""
        ids, sc = self.search(rq, pool)
        pc = self.prepared()
        Gs = []
        for q in range(ids.shape[0]):
            m = int((ids[q] != ID_NONE).sum())
            assert (ids[q, :m] != ID_NONE).all()                    # the filled slots are a prefix
            rows = np.ascontiguousarray(pc[(ids[q, :m] - np.uint64(self.offset)).astype(np.int64)]).reshape(m, self.dim)
            cols = np.asfortranarray(rows)                          # (the same values; the oracle walks column by column)
            Gs.append(O.numpy_scores_canonical(cols, cols, self.form))
        return ids, sc, Gs

    def select(self, pools, k, lam):
        """-> (ids uint64 [nq, k], scores float32 [nq, k], mmr float32 [nq, k]) in selection order."""
        ids, sc, Gs = pools
        nq = ids.shape[0]
        oi = np.full((nq, k), ID_NONE, np.uint64)
        osc = np.full((nq, k), np.nan, np.float32)
        omm = np.full((nq, k), np.nan, np.float32)
        for q in range(nq):
            m = Gs[q].shape[0]
            pos, v = greedy(sc[q, :m], Gs[q], k, lam, self.form == METRIC_L2)
            n = pos.size
            oi[q, :n], osc[q, :n], omm[q, :n] = ids[q, pos], sc[q, pos], v
        return oi, osc, omm

    def search_diverse(self, rq, k, pool, lam):
        return self.select(self.pools(rq, pool), k, lam)
