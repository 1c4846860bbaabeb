"""Row bitmaps of a mutable `Corpus` in the native library's form: uint32 words, bit i & 31 of
word i >> 5 for row i, zero bits beyond N.  Imports without the native library."""
from __future__ import annotations

import numpy as np


def words_for(n: int) -> int:
    return (int(n) + 31) // 32


def pack_mask(mask: np.ndarray) -> np.ndarray:
    """A bool array (N,) or (Q, N) as uint32 words (1, W) or (Q, W), W = ceil(N / 32)."""
    m = np.atleast_2d(np.asarray(mask, dtype=bool))
    rows, n = m.shape
    padded = np.zeros((rows, words_for(n) * 32), dtype=bool)
    padded[:, :n] = m
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32, copy=False)


def unpack_mask(words: np.ndarray, n: int) -> np.ndarray:
    """The first n bits of one row of words as a bool array (n,)."""
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[: int(n)].astype(bool)


def compaction_map(alive: np.ndarray) -> np.ndarray:
    """new_id_of_old (int64, one entry per row) of a compaction that keeps the live rows in order: -1 for a removed row."""
    a = np.asarray(alive, dtype=bool).reshape(-1)
    return np.where(a, np.cumsum(a, dtype=np.int64) - 1, np.int64(-1))
