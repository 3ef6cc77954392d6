"""The MFMA mutual-NN matching (csrc/matching.hip) against the oracle on the
winning 64-bit keys -- diff bits and index, not only the argmins -- on inputs
where a wrong kernel shows (tests/match_inputs.py): order-sensitive clustered
features, exact ties at every level of the kernel's reductions, n1 > 1024 in
the finalize kernel, every channel-count path, special values, and the
call's discipline on outputs, workspace and errors.  A key mismatch with an
equal argmin is a failure: the kernel is then not the chain that
include/pcr_math.h states."""
import functools

import numpy as np
import pytest
import torch

import oracle
import match_inputs as mi

pytestmark = pytest.mark.gpu

NAMES = ("corr12", "corr21", "idx1", "idx2", "count")
LAYOUTS = pytest.mark.parametrize("cm", [False, True], ids=["rowmajor", "chmajor"])


@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    """(f1, f2, the oracle's seven outputs) of one seeded input, built once
    for the row-major and the channel-major run"""
    if kind == "normal":
        p, n1, n2, c = args
        rng = np.random.default_rng(p * 7 + n1 + c)
        f1 = rng.standard_normal((p, n1, c), dtype=np.float32)
        f2 = rng.standard_normal((p, n2, c), dtype=np.float32)
    elif kind == "clustered":
        n1, n2, c = args
        f1, f2 = mi.clustered(n1, n2, c, seed=n1 + c)
    elif kind == "alphabet":
        n1, n2, c, lo, hi = args
        f1, f2 = mi.alphabet(n1, n2, c, lo, hi, seed=n1 + n2)
    elif kind == "permuted":
        p, n1, n2, c = args
        f1, f2 = mi.permuted_copy(n1, n2, c, seed=n1 + n2, p=p)
    elif kind == "special":
        f1, f2 = mi.special_values()[args[0]]
    elif kind == "self":
        f1, _ = mi.alphabet(300, 1, 4, -1, 2, seed=9)
        f2 = f1
    else:
        raise KeyError(kind)
    return f1, f2, oracle.mutual_nn_keys(f1, f2)


def _run(dev, f1, f2, cm=False):
    """ops.mutual_nn_match(return_keys=True) on numpy [p, n, c] features (the
    channel-major call gets their transposes) -> seven numpy arrays"""
    from pcr_amd import ops
    if cm:
        f1, f2 = f1.transpose(0, 2, 1), f2.transpose(0, 2, 1)
    t1 = torch.from_numpy(np.ascontiguousarray(f1)).to(dev)
    t2 = torch.from_numpy(np.ascontiguousarray(f2)).to(dev)
    got = ops.mutual_nn_match(t1, t2, channel_major=cm, return_keys=True)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _assert_equal(got, exp):
    mi.assert_keys_equal(got[5], exp[5], "rowbest")
    mi.assert_keys_equal(got[6], exp[6], "colbest")
    for g, e, name in zip(got, exp, NAMES):
        assert np.array_equal(g, e), name


def _check(dev, f1, f2, exp, cm=False):
    got = _run(dev, f1, f2, cm)
    _assert_equal(got, exp)
    return got


@LAYOUTS
@pytest.mark.parametrize("case", [("normal", 2, 300, 280, 64), ("clustered", 600, 600, 64),
                                  ("clustered", 257, 385, 33), ("normal", 1, 128, 128, 512)],
                         ids=lambda c: "-".join(map(str, c)))
def test_keys_match_oracle(dev, case, cm):
    """Diff bits of every winner: far-apart random features, the clustered
    inputs whose argmins move with the summation order (asserted in
    test_matching_cpu.py), and the 512-channel chain through 32 stages."""
    _check(dev, *_case(*case), cm=cm)


@LAYOUTS
@pytest.mark.parametrize("shape", mi.ALPHABET_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_exact_ties_take_the_first_index(dev, shape, cm):
    """Exact small-integer features: ties inside a lane's column pair, across
    lanes, halves, waves and tiles, for rows and columns alike."""
    _check(dev, *_case("alphabet", *shape), cm=cm)


@LAYOUTS
@pytest.mark.parametrize("zero", [True, False], ids=["zeros", "one_row"])
def test_degenerate_features(dev, zero, cm):
    """Every diff equal: index 0 wins every row and column, one mutual pair."""
    v = np.zeros(8, np.float32) if zero else \
        np.random.default_rng(2).standard_normal(8, dtype=np.float32)
    f1, f2 = np.tile(v, (1, 200, 1)), np.tile(v, (1, 300, 1))
    c12, c21, i1, i2, cnt, rb, cb = _run(dev, f1, f2, cm)
    assert np.all(c12 == 0) and np.all(c21 == 0) and cnt[0] == 1
    assert i1[0, 0] == 0 and i2[0, 0] == 0
    assert np.all(i1[0, 1:] == -1) and np.all(i2[0, 1:] == -1)
    exp = oracle.mutual_nn_keys(f1, f2)
    mi.assert_keys_equal(rb, exp[5], "rowbest")
    mi.assert_keys_equal(cb, exp[6], "colbest")


@LAYOUTS
def test_placed_column_ties(dev, cm):
    """Two equal f2 rows at the column strides of the row reduction: the
    lower column wins corr12."""
    a, b, rows, los = mi.placed_ties(mi.COLUMN_TIE_PAIRS)
    got = _check(dev, a, b, oracle.mutual_nn_keys(a, b), cm)
    assert np.array_equal(got[0][0, rows], los), list(zip(got[0][0, rows], mi.COLUMN_TIE_PAIRS))


@LAYOUTS
def test_placed_row_ties(dev, cm):
    """Two equal f1 rows at the row strides of the C/D layout and of the ti /
    wave / tile steps: the lower row wins corr21."""
    a, b, cols, los = mi.placed_ties(mi.ROW_TIE_PAIRS)
    got = _check(dev, b, a, oracle.mutual_nn_keys(b, a), cm)
    assert np.array_equal(got[1][0, cols], los), list(zip(got[1][0, cols], mi.ROW_TIE_PAIRS))


@pytest.mark.parametrize("p,n1,n2", [(1, 1025, 1), (1, 1, 2500), (1, 2500, 130), (1, 2049, 2049),
                                     (3, 1500, 257)])
def test_finalize_chunks_and_pair_stride(dev, p, n1, n2):
    """n1 > 1024: the finalize kernel's chunks carry the count of the mutual
    pairs found so far.  f2 / f1 is a permuted subset of the other side, so
    count == min(n1, n2) and the pairs spread over every chunk."""
    f1, f2, exp = _case("permuted", p, n1, n2, 4)
    got = _check(dev, f1, f2, exp)
    assert np.all(got[4] == min(n1, n2))
    if n1 > 1024 and n2 > 1:
        assert np.all((got[2][:, :min(n1, n2)] > 1024).any(axis=1))


@pytest.mark.parametrize("n1,n2", mi.TILE_EDGE_PAIRS)
def test_tile_and_half_edges(dev, n1, n2):
    f1, f2 = mi.clustered(n1, n2, 5, seed=n1)
    _check(dev, f1, f2, oracle.mutual_nn_keys(f1, f2))


@LAYOUTS
@pytest.mark.parametrize("c", [1, 2, 4, 7, 8, 12, 15, 16, 17, 20, 31, 32, 36])
def test_channel_counts(dev, c, cm):
    """The float4 path, the scalar tail and the stage boundary at 16: on the
    clustered input a channel dropped or doubled moves the keys."""
    _check(dev, *_case("clustered", 130, 70, c), cm=cm)


@LAYOUTS
@pytest.mark.parametrize("name", sorted(mi.special_values()))
def test_special_values(dev, name, cm):
    """NaN, infinities, overflowed norms and subnormal products through the
    device's branch-free key mapping (the expectations are written out by
    hand in test_matching_cpu.py::test_special_values_by_hand)."""
    _check(dev, *_case("special", name), cm=cm)


@LAYOUTS
def test_zero_diffs_on_identical_features(dev, cm):
    """f2 = f1 on the exact alphabet: the zero diffs of a row's copies tie and
    the first copy wins (no diff is ever -0: see test_matching_cpu.py)."""
    _check(dev, *_case("self"), cm=cm)


def test_unaligned_base_pointer(dev):
    """Features starting 4 bytes off a 16-byte boundary with c % 4 == 0: the
    float4 path's loads are dword-aligned only, which gfx950 global loads
    allow (include/pcr_amd.h)."""
    from pcr_amd import ops
    f1, f2 = mi.clustered(200, 150, 8, seed=4)
    exp = oracle.mutual_nn_keys(f1, f2)
    ts = []
    for f in (f1, f2):
        flat = torch.empty(f.size + 1, dtype=torch.float32, device=dev)
        t = flat[1:].view(f.shape)
        t.copy_(torch.from_numpy(f))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        ts.append(t)
    got = ops.mutual_nn_match(ts[0], ts[1], return_keys=True)
    torch.cuda.synchronize()
    _assert_equal([g.cpu().numpy() for g in got], exp)


# ---- the C ABI directly: poisoned outputs, workspace discipline, errors

class _Raw:
    """One pcr_mutual_nn_match call on outputs prefilled with 0x7f bytes"""

    def __init__(self, dev, p, n1, n2):
        self.p, self.n1, self.n2 = p, n1, n2
        self.outs = [torch.full(s, 0x7F7F7F7F, dtype=torch.int32, device=dev)
                     for s in ((max(p, 1), n1), (max(p, 1), n2), (max(p, 1), n1),
                               (max(p, 1), n1), (max(p, 1),))]

    def call(self, t1, t2, c, ws, ws_bytes=None, p=None, n2=None, c_arg=None, cm=False):
        from pcr_amd import _lib
        lib = _lib.load()
        fn = lib.pcr_mutual_nn_match_cm if cm else lib.pcr_mutual_nn_match
        st = fn(t1.data_ptr(), t2.data_ptr(), self.p if p is None else p, self.n1,
                self.n2 if n2 is None else n2, c if c_arg is None else c_arg,
                *[o.data_ptr() for o in self.outs], ws.data_ptr(),
                ws.numel() if ws_bytes is None else ws_bytes,
                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st

    def untouched(self):
        return all(bool((o == 0x7F7F7F7F).all()) for o in self.outs)

    def numpy(self):
        return [o[:self.p].cpu().numpy() for o in self.outs]


def _keys_of(ws, p, n1, n2):
    off = (p * n1 * 8 + 255) // 256 * 256
    w = ws.cpu().numpy()
    return (w[:p * n1 * 8].view(np.int64).reshape(p, n1),
            w[off:off + p * n2 * 8].view(np.int64).reshape(p, n2))


def test_outputs_and_workspace_discipline(dev):
    """Every output element is written (outputs start as 0x7f bytes, the
    workspace as random bytes); the keys sit where include/pcr_amd.h says;
    workspace bytes past them are never touched; a dirty, larger workspace
    reused for a smaller shape gives what a fresh call gives; two identical
    calls agree bit for bit (the order of the atomicMin merges must not
    show)."""
    from pcr_amd import _lib
    lib = _lib.load()
    p, n1, n2, c = 2, 300, 280, 16
    f1, f2 = mi.clustered(n1, n2, c, seed=21, p=p)
    exp = oracle.mutual_nn_keys(f1, f2)
    t1, t2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
    need = lib.pcr_mutual_nn_workspace_size(p, n1, n2)
    assert need == (p * n1 * 8 + 255) // 256 * 256 + (p * n2 * 8 + 255) // 256 * 256
    ws = torch.randint(0, 256, (need + 4096,), dtype=torch.uint8, device=dev)
    before = ws.clone()
    used = (p * n1 * 8 + 255) // 256 * 256 + p * n2 * 8
    runs = []
    for _ in range(2):
        raw = _Raw(dev, p, n1, n2)
        assert raw.call(t1, t2, c, ws) == 0
        runs.append(raw.numpy() + list(_keys_of(ws, p, n1, n2)))
        assert torch.equal(ws[used:], before[used:])
    _assert_equal(runs[0], exp)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # the same workspace, dirty with the keys of the larger call
    q1, q2, qc = 130, 70, 5
    g1, g2 = mi.clustered(q1, q2, qc, seed=22)
    raw = _Raw(dev, 1, q1, q2)
    assert raw.call(torch.from_numpy(g1).to(dev), torch.from_numpy(g2).to(dev), qc, ws) == 0
    _assert_equal(raw.numpy() + list(_keys_of(ws, 1, q1, q2)), oracle.mutual_nn_keys(g1, g2))
    assert torch.equal(ws[used:], before[used:])


def test_no_pairs_is_ok_and_writes_nothing(dev):
    from pcr_amd import ops
    t = torch.zeros((1, 8, 4), device=dev)
    ws = torch.full((512,), 0x5A, dtype=torch.uint8, device=dev)
    for cm in (False, True):
        raw = _Raw(dev, 0, 8, 8)
        assert raw.call(t, t, 4, ws, cm=cm) == 0
        assert raw.untouched() and bool((ws == 0x5A).all())
    got = ops.mutual_nn_match(t[:0], t[:0], return_keys=True)
    assert [tuple(g.shape) for g in got] == [(0, 8), (0, 8), (0, 8), (0, 8), (0,), (0, 8), (0, 8)]


def test_errors_leave_outputs_untouched(dev):
    from pcr_amd import _lib
    lib = _lib.load()
    p, n1, n2, c = 2, 130, 70, 4
    f1, f2 = mi.clustered(n1, n2, c, seed=23, p=p)
    t1, t2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
    need = lib.pcr_mutual_nn_workspace_size(p, n1, n2)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    for cm in (False, True):
        raw = _Raw(dev, p, n1, n2)
        assert raw.call(t1, t2, c, ws, ws_bytes=need - 1, cm=cm) < 0
        assert b"workspace too small" in lib.pcr_last_error()
        assert raw.call(t1, t2, c, ws, n2=0, cm=cm) < 0
        assert b"invalid sizes" in lib.pcr_last_error()
        assert raw.call(t1, t2, c, ws, c_arg=0, cm=cm) < 0
        assert b"invalid sizes" in lib.pcr_last_error()
        assert raw.untouched() and bool((ws == 0x5A).all())
    # the exact size is enough
    assert raw.call(t1, t2, c, ws) == 0
    _assert_equal(raw.numpy() + list(_keys_of(ws, p, n1, n2)), oracle.mutual_nn_keys(f1, f2))
