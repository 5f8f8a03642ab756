"""CPU guards for the LDS image of the nn/tn/tt GEMM (native/gemm_layout.hip).

An operand stored [K, X] has the K-tile [64 k-rows][128 x] bf16. lay_off
below is the Python twin of the kernel's image function; the tests replay
the staging and every ds_read_b64_tr_b16 the kernel issues — mechanism and
bank rule as documented for gfx950 — so an edit that breaks the fragment map
or the conflict-freedom fails without a GPU. The last tests cover the
stride-to-layout rule and the padded shapes of ops.matmul on CPU tensors.
"""

import pytest
import torch

ROWS, CHUNKS, TILE_BYTES = 64, 16, 64 * 256


def lay_key(row):
    return ((row & 3) << 2) | ((row >> 2) & 3)


def lay_off(row, ch):
    """byte offset of global 16-byte chunk ch of k-row `row`"""
    return 256 * row + 16 * (ch ^ lay_key(row))


def staged_image():
    """LDS byte -> (k-row, x) element it holds, by replaying the kernel's
    staging: 2 issues x 8 waves x 64 lanes, lane-linear 16-byte writes;
    the lane of LDS chunk slot s fetches global chunk (s&15) ^ key(s>>4)
    of row s>>4. Returns {element-aligned byte offset: (row, x)}."""
    image = {}
    for issue in range(2):
        for wid in range(8):
            o_base = issue * 512 * 8 + wid * 64 * 8        # elements
            rows_of_issue = set()
            for lane in range(64):
                slot = o_base // 8 + lane
                krow = slot >> 4
                x = 8 * ((slot & 15) ^ lay_key(krow))
                rows_of_issue.add(krow)
                byte = (o_base + lane * 8) * 2             # lane-linear
                for e in range(8):
                    assert byte + 2 * e not in image
                    image[byte + 2 * e] = (krow, x + e)
            # one wave issue = 4 whole rows
            assert len(rows_of_issue) == 4
            assert max(rows_of_issue) - min(rows_of_issue) == 3
    return image


def tr_reads():
    """Every transposed read of one K-tile: (side, x0, kk, block, addrs)
    with addrs[lane] for the 64 lanes. A side: wave row wr, m = 0..3
    (x0 = 64*wr + 16*m); B side: wave column wc, n = 0..1
    (x0 = 32*wc + 16*n). The eight waves are 2 (wr) x 4 (wc)."""
    x0s = {"A": sorted({64 * wr + 16 * m for wr in range(2)
                        for m in range(4)}),
           "B": sorted({32 * wc + 16 * n for wc in range(4)
                        for n in range(2)})}
    for side in ("A", "B"):
        assert x0s[side] == list(range(0, 128, 16))
        for x0 in x0s[side]:
            for kk in (0, 32):
                for block in (0, 1):
                    addrs = []
                    for lane in range(64):
                        g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
                        ch = (x0 >> 3) + (p >> 1)
                        row = kk + 8 * g + 4 * block + q
                        addrs.append(lay_off(row, ch) + 8 * (p & 1))
                    yield side, x0, kk, block, addrs


def test_off_is_a_row_preserving_bijection_in_chunks():
    offs = [lay_off(r, c) for r in range(ROWS) for c in range(CHUNKS)]
    assert sorted(offs) == list(range(0, TILE_BYTES, 16))
    for r in range(ROWS):
        for c in range(CHUNKS):
            assert lay_off(r, c) // 256 == r
            # an involution per row: LDS slot s holds global chunk s ^ key
            assert lay_off(r, (lay_off(r, c) % 256) // 16) == 256 * r + 16 * c


def test_staging_writes_the_image_off_describes():
    image = staged_image()
    assert sorted(image) == list(range(0, TILE_BYTES, 2))
    for r in range(ROWS):
        for x in range(128):
            assert image[lay_off(r, x >> 3) + 2 * (x & 7)] == (r, x)


def test_read_addresses_are_aligned_in_tile_and_row_contiguous():
    image = staged_image()
    count = 0
    for side, x0, kk, block, addrs in tr_reads():
        for lane, a in enumerate(addrs):
            assert a % 8 == 0 and 0 <= a and a + 8 <= TILE_BYTES
            row, x = image[a]
            assert [image[a + 2 * e] for e in range(4)] == \
                [(row, x + e) for e in range(4)], (side, x0, kk, block, lane)
        count += 1
    assert count == 2 * 8 * 2 * 2


def test_gather_reproduces_the_nt_fragment_map():
    """Per 16-lane group the instruction reads a 4 x 16 block — lane 4q+p
    addresses row q, columns 4p..4p+3 — and lane i receives column i, row
    q in element q. Two reads make the fragment: lane holds x = x0 +
    (lane&15), k = kk + 8*(lane>>4) + 0..7 in elements 0..7, which is what
    ds_read_b128 of a K-contiguous row gives the NT kernels."""
    image = staged_image()
    frags = {}
    for side, x0, kk, block, addrs in tr_reads():
        for g in range(4):
            blk = [[image[addrs[16 * g + 4 * q + p] + 2 * e]
                    for p in range(4) for e in range(4)] for q in range(4)]
            for i in range(16):
                lane = 16 * g + i
                for q in range(4):
                    frags[(side, x0, kk, lane, 4 * block + q)] = blk[q][i]
    assert len(frags) == 2 * 8 * 2 * 64 * 8
    for (side, x0, kk, lane, j), (row, x) in frags.items():
        assert x == x0 + (lane & 15)
        assert row == kk + 8 * (lane >> 4) + j


def test_every_transposed_read_is_conflict_free():
    """Bank of byte a is (a/4) % 64 and conflicts count per 32-lane half;
    a b64 read takes two consecutive banks per lane, so a half's 32 lanes
    must cover all 64 banks exactly once."""
    for side, x0, kk, block, addrs in tr_reads():
        for half in (addrs[:32], addrs[32:]):
            banks = [((a // 4) + d) % 64 for a in half for d in (0, 1)]
            assert sorted(banks) == list(range(64)), (side, x0, kk, block)


def test_without_the_key_the_reads_would_conflict():
    """The check above can tell: 256-byte rows all start on bank 0, so
    plain rows put a half's 8 rows on the same 8 banks."""
    addrs = [256 * (8 * (lane >> 4) + ((lane >> 2) & 3)) + 8 * (lane & 3)
             for lane in range(32)]
    banks = [((a // 4) + d) % 64 for a in addrs for d in (0, 1)]
    assert max(banks.count(b) for b in set(banks)) == 8


# ---- ops.matmul: strides -> layout, padded shapes (CPU tensors) -----------

def _ops():
    from hpc_patterns_amd import ops
    return ops


def test_layout_is_read_from_the_strides():
    ops = _ops()
    m, n, k = 5, 7, 3
    a_n, a_t = torch.zeros(m, k), torch.zeros(k, m).t()
    b_n, b_t = torch.zeros(k, n), torch.zeros(n, k).t()
    for a, b, want, sa, sb in ((a_n, b_n, "nn", (m, k), (k, n)),
                               (a_n, b_t, "nt", (m, k), (n, k)),
                               (a_t, b_n, "tn", (k, m), (k, n)),
                               (a_t, b_t, "tt", (k, m), (n, k))):
        layout, a_st, b_st = ops.matmul_layout(a, b)
        assert layout == want
        assert a_st.shape == sa and b_st.shape == sb
        assert a_st.is_contiguous() and b_st.is_contiguous()
        # views, never copies
        assert a_st.data_ptr() == a.data_ptr()
        assert b_st.data_ptr() == b.data_ptr()


def test_size_one_dimension_counts_as_row_major():
    ops = _ops()
    a = torch.zeros(4, 1).t()          # [1, 4]: strides fit both readings
    b = torch.zeros(1, 4).t()          # [4, 1]
    assert a.is_contiguous() and b.is_contiguous()
    layout, a_st, b_st = ops.matmul_layout(a, b)
    assert layout == "nn" and a_st.shape == (1, 4) and b_st.shape == (4, 1)


def test_other_strides_and_shapes_are_refused():
    ops = _ops()
    good = torch.zeros(6, 4)
    with pytest.raises(TypeError):     # a column slice: not dense
        ops.matmul_layout(torch.zeros(4, 12)[:, ::2], good)
    with pytest.raises(TypeError):     # the .t() of a row-strided view
        ops.matmul_layout(torch.zeros(12, 4)[::2].t(), torch.zeros(6, 4))
    with pytest.raises(TypeError):
        ops.matmul_layout(torch.zeros(2, 4, 6), good)
    with pytest.raises(ValueError):    # inner dimensions differ
        ops.matmul_layout(torch.zeros(4, 5), good)


def test_padded_shapes():
    ops = _ops()
    assert ops.gemm_layout_pad_shapes(100, 130, 70) == (128, 256, 128)
    assert ops.gemm_layout_pad_shapes(128, 128, 64) == (128, 128, 64)
    assert ops.gemm_layout_pad_shapes(1, 129, 65) == (128, 256, 128)
    assert ops.gemm_layout_pad_shapes(384, 640, 192) == (384, 640, 192)
