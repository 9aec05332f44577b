"""The host check that the per-pair kernels share (check_pair_table of csrc/qfx_pair_linalg.h), pinned through the four entry points
that every table builder calls: one list of malformed tables, and each of qfx_maxnorm_check_table, qfx_scaled_adamw_check_table,
qfx_lora_svd_check_table and qfx_lowrank_check_table refuses each of them; a well-formed table and the empty one are accepted.
The checks read the host table only, so the low-rank rows point at a dummy non-NULL address."""
import pytest

EINVAL = -1
I64_MAX = (1 << 63) - 1
DIM_MAX = 1 << 24
BIG = 1 << 40                                       # n_elems of the cases that are not about n_elems
CAPS = {"maxnorm": 128, "scaled_adamw": 64, "lora_svd": 64, "lowrank": 64}


def _check(kind, rows, n_elems, n=None):
    """rows: (off_a, off_b, r, in_features, out_features); the other fields of a row are well-formed."""
    from qflux_amd import _lib as L
    ctype, fill = {
        "maxnorm": (L.MaxnormPair, lambda r: r + (0.5,)),
        "scaled_adamw": (L.ScaledAdamwPair, lambda r: r + (1.0, 16.0, 0.0, 0.01, 0)),
        "lora_svd": (L.LoraSvdPair, lambda r: r + (0,)),
        "lowrank": (L.LowrankMat, lambda r: (0x1000, None, max(r[3], 1), 0) + r + (1, 0)),
    }[kind]
    arr = (ctype * len(rows))(*[ctype(*fill(tuple(r))) for r in rows]) if rows is not None else None
    return getattr(L.lib, f"qfx_{kind}_check_table")(arr, len(rows) if n is None else n, n_elems)


def _malformed(cap):
    """(label, rows, n_elems).  The well-formed pair is A [4, 16] at 0 and B [8, 4] at 64: 96 elements."""
    return [
        ("rank 0", [(0, 64, 0, 16, 8)], BIG),
        ("rank above the cap", [(0, 1 << 20, cap + 1, 16, 8)], BIG),
        ("in_features 0", [(0, 64, 4, 0, 8)], BIG),
        ("out_features 0", [(0, 64, 4, 16, 0)], BIG),
        ("in_features above 2^24", [(0, 1 << 30, 4, DIM_MAX + 1, 8)], BIG),
        ("out_features above 2^24", [(0, 1 << 30, 4, 16, DIM_MAX + 1)], BIG),
        ("negative off_a", [(-1, 64, 4, 16, 8)], BIG),
        ("negative off_b", [(0, -64, 4, 16, 8)], BIG),
        ("B past n_elems", [(0, 64, 4, 16, 8)], 95),
        ("A past n_elems", [(64, 0, 4, 16, 8)], 127),
        ("A overlaps B of its pair", [(0, 63, 4, 16, 8)], BIG),
        ("B of pair 1 overlaps A of pair 0", [(0, 500, 4, 16, 8), (1000, 40, 4, 16, 8)], BIG),
        ("off_a + n overflows int64", [(I64_MAX - 10, 64, 4, 16, 8)], I64_MAX),
        ("off_b + n overflows int64", [(0, I64_MAX - 10, 4, 16, 8)], I64_MAX),
    ]


@pytest.mark.parametrize("kind", sorted(CAPS))
def test_malformed_tables_are_refused(kind):
    for label, rows, n_elems in _malformed(CAPS[kind]):
        assert _check(kind, rows, n_elems) == EINVAL, (kind, label)
        if n_elems == BIG:                          # ... and also behind a well-formed pair that lies clear of the case's rows
            assert _check(kind, [(1 << 35, (1 << 35) + 64, 4, 16, 8)] + rows, BIG) == EINVAL, (kind, label, "behind a good row")


def test_project_check_reads_the_destination_spans():
    """qfx_lora_project_check_table goes through the same body with the spans of A' [r_dst, in] / B' [out, r_dst]: of the source
    row it tests the dimensions, not the offsets (those are qfx_lora_svd_check_table's to refuse)."""
    from qflux_amd import _lib as L
    pchk = L.lib.qfx_lora_project_check_table

    def check(src, dst, n_elems):
        return pchk((L.LoraSvdPair * 1)(L.LoraSvdPair(*src, 0)), (L.LoraSvdDst * 1)(L.LoraSvdDst(*dst)), 1, n_elems)

    good_src, good_dst = (0, 64, 4, 16, 8), (0, 64, 2, 4)           # A' [4, 16] at 0, B' [8, 4] at 64: 96 elements
    assert check(good_src, good_dst, 96) == 0 and check(good_src, good_dst, 95) == EINVAL
    assert check((-1, 64, 4, 16, 8), good_dst, 1000) == 0 and check((0, -64, 4, 16, 8), good_dst, 1000) == 0
    for src in ((0, 64, 0, 16, 8), (0, 64, 65, 16, 8), (0, 64, 4, 0, 8), (0, 64, 4, DIM_MAX + 1, 8), (0, 64, 4, 16, 0),
                (0, 64, 4, 16, DIM_MAX + 1)):
        assert check(src, good_dst, BIG) == EINVAL, src
    for dst in ((-1, 64, 2, 4), (0, -64, 2, 4), (0, 63, 2, 4), (I64_MAX - 10, 64, 2, 4), (0, 64, 0, 4), (0, 64, 5, 5), (0, 64, 2, 1),
                (0, 64, 2, 65)):
        assert check(good_src, dst, I64_MAX if dst[0] > BIG else BIG) == EINVAL, dst


@pytest.mark.parametrize("kind", sorted(CAPS))
def test_well_formed_tables_are_accepted(kind):
    cap = CAPS[kind]
    good = [(0, 64, 4, 16, 8), (100, 100 + cap, cap, 1, 1)]          # the second pair at the rank cap: A and B of cap elements each
    assert _check(kind, good, 100 + 2 * cap) == 0
    assert _check(kind, good, 100 + 2 * cap - 1) == EINVAL          # the extent is exact
    assert _check(kind, [(96, 0, 4, 16, 8), (32, 160, 4, 16, 8)], 192) == 0      # adjacent spans in any order do not overlap
    assert _check(kind, [(0, 1 << 30, 64, DIM_MAX, DIM_MAX)], 1 << 31) == 0       # the largest matrices
    assert _check(kind, None, 0, n=0) == 0                           # no pairs, no table
    assert _check(kind, None, 10, n=1) == EINVAL and _check(kind, good, 100 + 2 * cap, n=-1) == EINVAL and _check(kind, good, -1) == EINVAL
