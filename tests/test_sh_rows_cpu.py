"""CPU checks of the SH-row LDS layout (reduced-3dgs_amd/csrc/sh_rows.h): the index functions the staging code and the row
accessor share run on the host through tests/hostcheck_sh_rows and are checked EXHAUSTIVELY over everything a kernel can pass
-- every stride M, every row count of a wave, every float of both split spans -- against the plain definition of the layout
(divisions and remainders in Python integers).  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_sh_rows", "hostcheck_sh_rows.hip")
SO = os.path.join(HERE, "hostcheck_sh_rows", "libhostcheck_sh_rows.so")
# preprocess.hip kQuantSpanChunks: the 16-byte chunks that cover 64 rows of 48 id bytes starting at any byte of a chunk
QUANT_SPAN_CHUNKS = (64 * 48 + 15 + 15) // 16 + 1


@pytest.fixture(scope="module")
def lib():
    return build_shim(SRC, SO, EXACT, "hipcc not available to build the SH-row host-check shim")


def _skew(lib, rows48, n, first=0):
    out = np.full(n, -1, np.int32)
    lib.hs_skew(int(rows48), first, n, out.ctypes.data_as(C.c_void_p))
    return out.astype(np.int64)


def _split(lib, rows48, n, rl, k0, M):
    out = np.full(n, -1, np.int32)
    lib.hs_split_index(int(rows48), n, rl, k0, M, out.ctypes.data_as(C.c_void_p))
    return out.astype(np.int64)


def test_constants(lib):
    assert lib.hs_row_floats() == 48
    assert lib.hs_window_floats() == 64 * 48 + 64 * 48 // 32 == 3168


def test_dense_maps_are_injective_and_inside_the_window(lib):
    window = lib.hs_window_floats()
    general, rows48 = _skew(lib, False, 64 * 48), _skew(lib, True, 64 * 48)
    assert np.array_equal(general, np.arange(64 * 48) + np.arange(64 * 48) // 32)
    for M in range(1, 17):
        for nrows in range(1, 65):
            idx = general[:nrows * 3 * M]
            assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < window, (M, nrows)
    for nrows in range(1, 65):   # the ROWS48 form exists at M = 16 only
        idx = rows48[:nrows * 48]
        assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < window, nrows


def test_rows48_puts_rows_49_words_apart(lib):
    got = _skew(lib, True, 64 * 48).reshape(64, 48)
    r, k = np.meshgrid(np.arange(64), np.arange(48), indexing="ij")
    assert np.array_equal(got, 49 * r + k)


@pytest.mark.parametrize("rows48", [False, True])
def test_split_index_is_the_dense_index_of_the_joined_element(lib, rows48):
    for M in ([16] if rows48 else range(1, 17)):
        dense = _skew(lib, rows48, 64 * 3 * M)
        for rl, k0 in ((3, 0), (3 * (M - 1), 3)):
            if rl == 0:   # M = 1: there is no rest span
                continue
            n = 64 * rl   # every float of the span of a full wave: f < 64 * 45
            f = np.arange(n)
            joined = (f // rl) * 3 * M + k0 + f % rl
            assert np.array_equal(_split(lib, rows48, n, rl, k0, M), dense[joined]), (M, rl, k0)


def test_quantised_window_chunks_stay_in_one_skew_step(lib):
    """preprocess.hip color_role_quant stores the four words of chunk c at sh_skew<false>(4c) + 0..3."""
    words = _skew(lib, False, 4 * QUANT_SPAN_CHUNKS).reshape(QUANT_SPAN_CHUNKS, 4)
    assert np.array_equal(words, words[:, :1] + np.arange(4))
    assert len(np.unique(words)) == words.size
