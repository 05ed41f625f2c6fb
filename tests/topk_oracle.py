"""numpy restatement of the top-k selection of include/hidegs_topk.h (test infrastructure): the order key, the
mask by a stable argsort, and the four info words."""
import numpy as np


def ord_key(x):
    """u32 order keys of float32 scores: NaN -> 0, -0.0 as +0.0, otherwise (b >> 31) ? ~b : b | 0x80000000."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    key = np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0
    return key


def candidates(n, among):
    return np.ones(n, dtype=bool) if among is None else np.asarray(among).view(np.uint8) != 0


class Ranking:
    """The candidates of one input in selection order, computed once for many k."""

    def __init__(self, x, among=None):
        x = np.asarray(x, dtype=np.float32)
        self.n = x.size
        self.idx = np.nonzero(candidates(x.size, among))[0]
        keys = ord_key(x)[self.idx]
        self.order = np.argsort(~keys, kind="stable")
        self.keys = keys[self.order]  # descending
        self.c = int(self.idx.size)

    def mask(self, k):
        mask = np.zeros(self.n, dtype=bool)
        mask[self.idx[self.order[:min(int(k), self.c)]]] = True
        return mask

    def info(self, k):
        """[selected, candidates, threshold score bits, tie quota] as Python ints (unsigned)."""
        sel = min(int(k), self.c)
        if sel == 0:
            return [0, self.c, 0, 0]
        t = self.keys[sel - 1]
        above = int(np.searchsorted(-self.keys.astype(np.int64), -int(t), side="left"))  # keys > t
        return [sel, self.c, score_bits_of_key(t), sel - above]


def score_bits_of_key(key):
    """The canonical score bits of a key: +0.0 for a zero, 0x7FC00000 for a NaN."""
    key = int(key)
    if key == 0:
        return 0x7FC00000
    return key & 0x7FFFFFFF if key >> 31 else ~key & 0xFFFFFFFF


def top_k_mask(x, k, among=None):
    """bool (n,): the first min(k, c) candidates by descending key, then ascending row index:
    idx = nonzero(candidates), order = argsort(~ord_key(x)[idx], kind="stable"), set idx[order[:min(k, len(idx))]]."""
    return Ranking(x, among).mask(k)


def info_words(x, k, among=None):
    return Ranking(x, among).info(k)
