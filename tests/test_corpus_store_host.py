"""The mutable Corpus's host-side bitmap helpers (oscillink_amd/_masks.py) against bit-by-bit loops.  No GPU, no native
library."""
import numpy as np
import pytest

from oscillink_amd import _masks as mk


def _pack_by_loop(mask):
    m = np.atleast_2d(mask)
    words = np.zeros((m.shape[0], (m.shape[1] + 31) // 32), dtype=np.uint32)
    for q in range(m.shape[0]):
        for i in range(m.shape[1]):
            if m[q, i]:
                words[q, i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1100])
def test_pack_mask_matches_a_bit_by_bit_loop(N):
    rng = np.random.default_rng(N)
    for mask in (rng.random(N) < 0.5, np.ones(N, dtype=bool), np.zeros(N, dtype=bool), rng.random((3, N)) < 0.3):
        words = mk.pack_mask(mask)
        assert words.dtype == np.uint32 and words.flags.c_contiguous
        assert words.shape == (1 if mask.ndim == 1 else 3, mk.words_for(N))
        np.testing.assert_array_equal(words, _pack_by_loop(mask))
        for q in range(words.shape[0]):  # zero bits beyond N, and the way back
            assert int(words[q, -1]) >> ((N - 1) % 32 + 1) == 0
            np.testing.assert_array_equal(mk.unpack_mask(words[q], N), np.atleast_2d(mask)[q])


def test_words_for():
    assert [mk.words_for(n) for n in (0, 1, 31, 32, 33, 64, 65, 1100)] == [0, 1, 1, 1, 2, 2, 3, 35]


def test_compaction_map_keeps_order_and_marks_removed_rows():
    rng = np.random.default_rng(7)
    for N in (1, 5, 33, 1100):
        for alive in (rng.random(N) < 0.6, np.ones(N, dtype=bool), np.zeros(N, dtype=bool)):
            got = mk.compaction_map(alive)
            want, nxt = [], 0
            for a in alive:
                want.append(nxt if a else -1)
                nxt += int(a)
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, np.array(want, dtype=np.int64))
            np.testing.assert_array_equal(np.flatnonzero(got >= 0), np.flatnonzero(alive))  # old ids of the new rows
