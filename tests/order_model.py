"""rowpred_model.RowPredModelIndex with ordered selection: what vrod_index_select_ordered must return.

The rows considered are `matching(pred, flags & ALLOWED)`, the rows select_where lists.  Their order is (value, id)
ascending, or under DESC value descending and id still ascending; numpy.lexsort gives it.  A cursor (value, id) keeps
the rows strictly after it in that order -- it need not name a row.  The first `limit` of what is left are the result,
`total` counts all of it.
"""
import numpy as np

from index_model import ERR_INVALID_ARG, ModelError
from rowpred_model import ALLOWED, RowPredModelIndex

DESC = 2                                             # VROD_ORDER_DESC
MAX_ORDERED = 65536                                  # VROD_MAX_ORDERED


class OrderModelIndex(RowPredModelIndex):
    def select_ordered(self, pred, limit, desc=False, after=None, flags=0):
        """-> (ids uint64, values int64, total)."""
        if flags & ~(ALLOWED | DESC) or not 0 <= int(limit) <= MAX_ORDERED:
            raise ModelError(ERR_INVALID_ARG, "unknown flag bits, or a limit beyond MAX_ORDERED")
        desc = bool(desc) or bool(flags & DESC)
        rows = self.matching(pred, flags & ALLOWED)
        ids = rows.astype(np.uint64) + np.uint64(self.offset)
        vals = self.values[rows].astype(np.int64)
        if after is not None:
            cv, cid = np.int64(int(after[0])), np.uint64(int(after[1]))
            beyond = (vals < cv) if desc else (vals > cv)
            keep = beyond | ((vals == cv) & (ids > cid))
            ids, vals = ids[keep], vals[keep]
        # lexsort sorts by its LAST key first: the value (descending as the ascending order of its complement, which
        # unlike negation cannot overflow), then the id
        order = np.lexsort((ids, ~vals if desc else vals))
        total = int(order.size)
        order = order[:int(limit)]
        return ids[order], vals[order], total

    def scroll(self, pred, page, desc=False, flags=0):
        """The pages a caller gets who passes the last (value, id) of each page as the cursor of the next."""
        after = None
        while True:
            ids, vals, total = self.select_ordered(pred, page, desc, after, flags)
            if ids.size:
                yield ids, vals
            if total <= ids.size:
                return
            after = (int(vals[-1]), int(ids[-1]))
