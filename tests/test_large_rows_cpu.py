"""tests/large_rows.py on the CPU, with 2^9 .. 2^12 standing in for the boundaries 2^29 .. 2^32: the marker rows, the row count, the periodic
fill, that the periodic check finds a single wrong element, a row that took another row's place and a read displaced by a wrapped power of
two, and that the canary margins find a store before, behind and missing from an output."""
import pytest
import torch

import large_rows as LR

SMALL = (1 << 9, 1 << 10, 1 << 11, 1 << 12)


def test_boundary_rows_contain_each_boundary_with_neighbours():
    R, B = 40, LR.rows_for(40, target=1 << 12)
    rows = LR.boundary_rows(R, B, SMALL)
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == B - 1
    for T in SMALL:
        b = T // R
        assert b * R <= T < (b + 1) * R and {b - 1, b, b + 1} <= set(rows)
    assert len(rows) == 14                                   # 4 x 3 + row 0 + row B - 1: none coincide at this R
    assert LR.boundary_rows(R, 20, SMALL) == [0, 11, 12, 13, 19]        # boundaries past the tensor add nothing


def test_rows_for_is_the_smallest_count_with_both_neighbours():
    for R in (40, 24, 3, 163840 // 64):
        B = LR.rows_for(R, target=1 << 12)
        assert B * R >= (1 << 12) + 2 * R > (B - 1) * R
        assert (1 << 12) // R + 1 <= B - 1                   # the neighbour behind the last boundary row exists
    assert LR.rows_for(40, target=1 << 12, multiple=3) % 3 == 0
    # the shipped level-0 plane set: 26 217 rows, residues of the four boundaries inside their rows
    R = 40 * 64 * 64
    assert LR.rows_for(R) == 26217 and [T % R for T in LR.BOUNDARIES] == [131072, 98304, 32768, 65536]
    with pytest.raises(AssertionError, match="power of two"):
        LR.rows_for(64, target=1 << 12)
    with pytest.raises(AssertionError, match="limit"):
        LR.rows_for(3, target=1 << 12, limit=1000)
    with pytest.raises(AssertionError, match="limit"):
        LR.rows_for(R, limit=LR.CANDIDATE_LIMIT)


def _filled(R=40):
    B = LR.rows_for(R, target=1 << 12)
    markers = LR.boundary_rows(R, B, SMALL)
    g = torch.Generator().manual_seed(1)
    base = torch.randn(LR.P, R, generator=g)
    return LR.periodic_fill(torch.empty(B, R), base, markers, g), base, markers


def test_periodic_fill_and_base_rows():
    big, base, markers = _filled()
    for b in range(big.shape[0]):
        if b in markers:
            assert not any(torch.equal(big[b], base[r]) for r in range(LR.P))
        else:
            assert torch.equal(big[b], base[b % LR.P])
    assert len({tuple(big[m].tolist()) for m in markers}) == len(markers)          # each marker row has content of its own
    refs = LR.base_rows(LR.P, markers, big.shape[0])
    assert refs[0] == 5 and refs[1:] == [1, 2, 3, 4]                                # row 0 is a marker: residue 0 starts at row P
    assert LR.check_periodic(big, LR.P, markers) == refs


def test_check_periodic_finds_what_a_wrong_address_does(monkeypatch):
    big, base, markers = _filled()
    B, R = big.shape
    for slab in (LR.SLAB, 7 * R):                                                   # one slab, and many with a ragged last one
        monkeypatch.setattr(LR, "SLAB", slab)
        LR.check_periodic(big, LR.P, markers)
        one = big.clone()
        one[57, 13] += 1e-3                                                         # one element
        with pytest.raises(AssertionError, match=r"first: \[57\]"):
            LR.check_periodic(one, LR.P, markers)
        LR.check_periodic(one, LR.P, markers, exact=False, atol=2e-3)
        swapped = big.clone()
        swapped[33] = big[34]                                                       # a row from the neighbouring batch base
        with pytest.raises(AssertionError, match=r"\[33\]"):
            LR.check_periodic(swapped, LR.P, markers)
        wrapped = big.clone()                                                       # an element index that lost bit 9
        flat, src = wrapped.view(-1), big.view(-1)
        flat[600:640] = src[600 - 512:640 - 512]
        with pytest.raises(AssertionError, match="differ"):
            LR.check_periodic(wrapped, LR.P, markers)
        marker = big.clone()
        marker[markers[3]] = 0                                                      # marker rows are the caller's to check
        LR.check_periodic(marker, LR.P, markers)


def test_canaries_find_stores_outside_and_missing(monkeypatch):
    def op(before=False, behind=False, skip=False, scratch=False):
        out = torch.empty(6, 7, dtype=torch.float32)
        buf = out.view(-1)
        buf[:] = 1.0
        base = buf.as_strided((buf.numel() + 2,), (1,), buf.storage_offset() - 1)
        if before:
            base[0] = 2.0
        if behind:
            base[-1] = 2.0
        if skip:
            buf[11] = LR.CANARY
        if scratch:
            torch.empty((4,), dtype=torch.float64)
        return out

    with LR.canaries(monkeypatch):
        assert op().shape == (6, 7)
    for kw, msg in ((dict(before=True), "outside"), (dict(behind=True), "outside"), (dict(skip=True), "never written"), (dict(scratch=True), "never written")):
        with pytest.raises(AssertionError, match=msg):
            with LR.canaries(monkeypatch):
                op(**kw)
    got = []
    with LR.canaries(monkeypatch, got):                                             # a scratch buffer may stay unwritten when the results are named
        got.append(op(scratch=True))
    with pytest.raises(AssertionError, match="never written"):
        with LR.canaries(monkeypatch, got):
            got[:] = [op(skip=True)]
    with pytest.raises(AssertionError, match="no output"):
        with LR.canaries(monkeypatch):
            pass
    assert torch.empty(3).shape == (3,)                                             # the patch is gone


def test_need_bytes_counts_tensors_margins_and_temporaries():
    assert LR.need_bytes(1 << 32, 1 << 30) == 4 * ((1 << 32) + (1 << 30)) + 2 * 2 * LR.PAD * 4 + (2 << 30)
    assert LR.need_bytes(10, itemsize=8, temporaries=0) == 80 + 2 * LR.PAD * 8
