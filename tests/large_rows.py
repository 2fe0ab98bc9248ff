"""Helpers for tests/test_large_tensors_gpu.py: tensors of 2^29 .. 2^32 elements whose every row is checked with a reference for a
handful of rows only.

A (B, ...) tensor with R elements per row is filled periodically: row b holds base[b % P], except the marker rows -- the rows that
contain element 2^29, 2^30, 2^31 or 2^32 (where a signed / unsigned 32-bit byte offset and a signed / unsigned 32-bit element index
break), their two neighbours, row 0 and row B - 1 -- which each get content of their own.  An op that works row by row then has a
periodic output: every non-marker row must equal the first non-marker row of its residue class, and only those P rows and the markers
need a reference.  R must have an odd prime factor: then no power of two is a multiple of R, an access displaced by a wrapped 2^k lands
in the middle of a row and cannot hit an equal one.

Plain torch, no kernels of the project: tests/test_large_rows_cpu.py runs all of it on the CPU with 2^9 .. 2^12 as the boundaries."""
import contextlib

import pytest
import torch

BOUNDARIES = (1 << 29, 1 << 30, 1 << 31, 1 << 32)
P = 5
ROW_LIMIT = 65535                # launch-grid y / z extent: rows per call of most ops
CANDIDATE_LIMIT = 21845          # candidate_finalize: three planes per candidate in grid.y
CANARY, PAD = 12345.0, 1 << 15
BYTE_CANARY = 0x5A               # for the byte workspaces some ops allocate like their results
SLAB = 1 << 28                   # elements compared at a time: a bool temporary of 256 MiB, a float one of 1 GiB
MEMORY_LIMIT = 64 << 30


def boundary_rows(R, B, boundaries=BOUNDARIES):
    """The rows of a (B, ...) tensor with R elements per row that contain element index T for T in boundaries (those inside the tensor), their
    two neighbours, row 0 and row B - 1; sorted."""
    rows = {0, B - 1}
    for T in boundaries:
        b = T // R
        if b < B:
            rows.update(r for r in (b - 1, b, b + 1) if 0 <= r < B)
    return sorted(rows)


def rows_for(R, target=1 << 32, limit=ROW_LIMIT, multiple=1):
    """The smallest B (a multiple of ``multiple``) with B R >= target + 2 R: the boundary row and both neighbours exist."""
    assert R > 0 and R & (R - 1), f"R = {R} is a power of two: a wrapped 2^k offset would land on the same place of another row"
    B = -(-(target + 2 * R) // R)
    B = -(-B // multiple) * multiple
    assert B <= limit, f"{B} rows of {R} elements: above the op's limit of {limit} rows per call"
    return B


def fresh_normal(gen, n, shape):
    return torch.randn(n, *shape, generator=gen)


def periodic_fill(big, base, markers, gen, fresh=fresh_normal):
    """big[b] = base[b % P] with P = len(base), except big[m] = content of its own for m in markers (``fresh(gen, n, row shape)``, a CPU tensor)."""
    B, period = big.shape[0], base.shape[0]
    n = B // period
    base = base.to(big.device, big.dtype)
    if n:
        big[:n * period].view(n, period, *big.shape[1:]).copy_(base.unsqueeze(0).expand(n, *base.shape))
    if B % period:
        big[n * period:].copy_(base[:B % period])
    new = fresh(gen, len(markers), tuple(big.shape[1:])).to(big.device, big.dtype)
    for i, m in enumerate(markers):
        big[m].copy_(new[i])
    return big


def base_rows(period, markers, B):
    """For each residue r < period the first row b = r (mod period) that is no marker: the row every other one of its class must equal."""
    mk, rows = set(markers), []
    for r in range(period):
        b = r
        while b in mk:
            b += period
        assert b < B, f"every row of residue {r} is a marker"
        rows.append(b)
    return rows


def _rows_equal(a, b, exact, rtol, atol):
    if exact:
        return (a == b).all(-1)
    return torch.isclose(a, b, rtol=rtol, atol=atol).all(-1)


def check_periodic(out, period, markers, exact=True, rtol=0.0, atol=0.0):
    """Every non-marker row of out (B, ...) equals the base row of its residue class (bit for bit, or within rtol / atol where the op
    accumulates with float atomics); compared in slabs of at most SLAB elements.  Returns the base rows."""
    B = out.shape[0]
    flat = out.reshape(B, -1)
    R = flat.shape[1]
    mk = set(markers)
    refs = base_rows(period, markers, B)
    ref = torch.stack([flat[b] for b in refs])
    per = max(1, SLAB // max(R, 1) // period) * period
    bad = []
    for s in range(0, B, per):
        e = min(B, s + per)
        n = (e - s) // period
        ok = []
        if n:
            ok.append(_rows_equal(flat[s:s + n * period].view(n, period, R), ref.unsqueeze(0), exact, rtol, atol).reshape(-1))
        if s + n * period < e:
            ok.append(_rows_equal(flat[s + n * period:e], ref[:e - s - n * period], exact, rtol, atol))
        wrong = torch.nonzero(~torch.cat(ok)).flatten().tolist()
        bad += [s + i for i in wrong if s + i not in mk]
    assert not bad, f"{len(bad)} rows differ from the base row of their residue class (period {period}); the first: {bad[:8]}"
    return refs


def _slabs(t):
    flat = t.reshape(-1)
    for s in range(0, flat.numel(), SLAB):
        yield flat[s:s + SLAB]


@contextlib.contextmanager
def canaries(monkeypatch, returned=None):
    """Every tensor the op allocates for its results (torch.empty / torch.empty_like) becomes a view into the middle of a larger buffer
    filled with CANARY; on exit the margins on both sides must still hold it and no element in between may.  ``returned``: a list the
    caller fills, inside the block, with the tensors the op returned -- then only these must be written everywhere (an op's scratch
    buffers, allocated the same way, keep the canary where the op has nothing to write), the margins of all are still checked.
    Where the op writes into a tensor of the caller that the caller has filled first (copy_channels, add_channels, transpose_planes_into), no
    canary is left inside it: for those only the margins are watched here, and what lies inside is the comparisons' to judge."""
    bufs = []

    def inside(shape, device, dtype):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = 1
        for s in shape:
            n *= int(s)
        canary = BYTE_CANARY if dtype in (torch.uint8, torch.int8) else CANARY
        buf = torch.full((n + 2 * PAD,), canary, device=device, dtype=dtype)
        bufs.append((buf, n, canary))
        return buf[PAD:PAD + n].view(*shape)

    with monkeypatch.context() as m:
        m.setattr(torch, "empty_like", lambda t, **_: inside(t.shape, t.device, t.dtype))
        m.setattr(torch, "empty", lambda *shape, device=None, dtype=None, **_: inside(shape, device, dtype))
        yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    assert bufs, "the op allocated no output"
    ptrs = None if returned is None else {t.data_ptr() for t in returned}
    assert ptrs is None or ptrs, "the caller named no returned tensor"
    for buf, n, canary in bufs:
        assert bool((buf[:PAD] == canary).all()) and bool((buf[PAD + n:] == canary).all()), "a store landed outside the output tensor"
        if ptrs is None or buf[PAD:].data_ptr() in ptrs:
            assert not any(bool((s == canary).any()) for s in _slabs(buf[PAD:PAD + n])), "an output element was never written"


def need_bytes(*numels, itemsize=4, temporaries=2 << 30):
    """Peak device bytes of a case: its large tensors (element counts; the canary margins are included) and the slab temporaries of the checks."""
    return sum(int(n) * itemsize + 2 * PAD * itemsize for n in numels) + temporaries


def require_memory(need):
    """The case's peak must stay within MEMORY_LIMIT; skips (with the figures) where the device has less than that free."""
    assert need <= MEMORY_LIMIT, f"the case needs {need / 2**30:.1f} GiB, above the {MEMORY_LIMIT >> 30} GiB a test may take"
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB are free")
