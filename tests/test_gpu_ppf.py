"""The five PPF kernels of csrc/local_ppf.hip, bit for bit against the oracle
and within the project's bounds of an independent float64 restatement
(tests/ppf_restate.py), where they can go wrong unseen:

 - the shared-reciprocal division of ppf_local_dev at the edges of its
   [2^-60, 2^60] range, safe and unsafe lanes in one wave, relative = 0 and 1;
 - unit, zero, NaN, inf, tiny and huge normals and cosines planted at +-1 and
   on the +-0.5 seam of the acos selects;
 - the dispatch lines of pcr_knn_ppf_sorted: quad / cloud kernel, one or two
   point ranges, odd k, n < k, the XCD remap, caller pointers that are not
   16-byte aligned;
 - the explicit-index kernels at point, slot and layout tails, n != m,
   out-of-range ids, and their choice by pointer equality;
 - the global PPF at its 1e-10 and 1e-20 thresholds.

Every output buffer is poisoned first (ids -7, PPF NaN, workspace 0xA5).
test_ppf_cpu.py pins the properties of the inputs used here."""
import numpy as np
import pytest

import ppf_restate as R

pytestmark = pytest.mark.gpu

MARGIN = 4  # guard elements on either side of a buffer's view (16 bytes)


def T(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the cases are read-only


def N(t):
    return t.detach().cpu().numpy()


def guarded(dev, shape, dtype, poison, off=0, data=None):
    """A contiguous view of `shape` inside a poisoned flat buffer, starting
    MARGIN + off elements in: 16-byte aligned for off = 0, only 4-byte aligned
    for off = 1.  -> (buffer, view)."""
    import torch
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * MARGIN,), poison, dtype=dtype, device=dev)
    view = buf[MARGIN + off:MARGIN + off + numel].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    if data is not None:
        view.copy_(T(data, dev))
    return buf, view


def guards_intact(buf, view, poison):
    """The elements before and after the view still hold their poison."""
    g = N(buf)
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    edge = np.concatenate([g[:lo], g[lo + view.numel():]])
    assert edge.size == 2 * MARGIN
    return np.isnan(edge).all() if poison != poison else (edge == poison).all()


def run_sorted(dev, xyz, nrm, k, relative, off=(0, 0, 0, 0)):
    """pcr_knn_prepare + pcr_knn_select_ppf; `off` shifts xyz, normals, idx
    and ppf by that many elements off 16-byte alignment.  -> (idx, ppf)."""
    import torch
    from pcr_amd import _lib
    from pcr_amd.ops import _ptr, _stream
    b, _, n = xyz.shape
    nan = float("nan")
    _, tx = guarded(dev, xyz.shape, torch.float32, nan, off[0], xyz)
    _, tn = guarded(dev, nrm.shape, torch.float32, nan, off[1], nrm)
    bi, idx = guarded(dev, (b, k, n), torch.int32, -7, off[2])
    bp, ppf = guarded(dev, (b, 4, k, n), torch.float32, nan, off[3])
    lib = _lib.load()
    ws = torch.full((lib.pcr_knn_workspace_size(b, n, n),), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.pcr_knn_prepare(_ptr(tx), b, n, _ptr(ws), ws.numel(), _stream()), "prepare")
    _lib.check(lib.pcr_knn_select_ppf(_ptr(tx), _ptr(tn), b, n, k, int(relative), _ptr(idx),
                                      _ptr(ppf), _ptr(ws), ws.numel(), _stream()), "select_ppf")
    torch.cuda.synchronize()
    assert guards_intact(bi, idx, -7), "idx written outside its view"
    assert guards_intact(bp, ppf, nan), "ppf written outside its view"
    return N(idx), N(ppf)


def assert_ids(got, exp):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "idx differs at %d places, first %s: got %s exp %s" % (
        len(bad), bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def assert_bits(got, exp, what="ppf"):
    if np.array_equal(got, exp, equal_nan=True):
        return
    bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    raise AssertionError("%s differs at %d of %d places, first %s: got %r exp %r" % (
        what, len(bad), got.size, bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])]))


def check_sorted_case(dev, name, relative, off=(0, 0, 0, 0)):
    xyz, nrm, k, ids, ppf = R.sorted_case(name, relative)
    gi, gp = run_sorted(dev, xyz, nrm, k, relative, off)
    assert_ids(gi, ids)
    assert_bits(gp, ppf)
    return gi, gp


# ----------------------------------- 2. shared reciprocal at its range edges
@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("name", R.SCALE_CASES)
def test_sorted_ppf_at_range_edges(dev, name, relative):
    """Clouds scaled by 2^-61 .. 2^-59 and 2^58 .. 2^60 (and 1), a lattice
    whose d components land on and around 2^-60, and one cloud mixing both:
    n = 1024 runs local_ppf_quad_kernel, n = 1023 local_ppf_cloud_kernel, both
    over two point ranges; family B (n = 516) the quad kernel."""
    _, gp = check_sorted_case(dev, name, relative)
    R.check_sorted_case_f64(name, relative, out=gp)


# ------------------------------------------ 3. normals and the acos selects
@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("n", R.NORMAL_SIZES)
def test_sorted_ppf_normals_and_acos_seams(dev, n, relative):
    """Unit normals; unit normals with zero, NaN, inf, 1e-20 and 1e20 rows and
    cosines planted at +-1 and +-0.5; np.roll normals (heavy clamping)."""
    name = "normals-n%d" % n
    _, gp = check_sorted_case(dev, name, relative)
    R.check_sorted_case_f64(name, relative, out=gp)


# ------------------------------- 4. dispatch lines of pcr_knn_ppf_sorted
@pytest.mark.parametrize("name", R.SIZE_CASES)
def test_sorted_ppf_dispatch_sizes(dev, name):
    """pr flips at 513; 516 = 260 + 256 and 1020 = 512 + 508 quad ranges;
    1028 and 2048 the quad kernel over one range; 2045 the cloud kernel at
    nearly its largest LDS footprint; 4 and 5 leave unfilled slots; k = 31
    ends on a one-slot group; b = 3, k = 7, n = 516 is 24 workgroups through
    the XCD remap."""
    _, gp = check_sorted_case(dev, name, 1)
    R.check_sorted_case_f64(name, 1, out=gp)


OFFSETS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("off", OFFSETS, ids=["xyz", "normals", "idx", "ppf", "all"])
@pytest.mark.parametrize("n", [1024, 516])
def test_sorted_ppf_unaligned_pointers(dev, n, off):
    """n % 4 == 0 with a caller pointer off 16-byte alignment: the v16 test
    sends these to local_ppf_cloud_kernel<2, 4> (4-byte accesses only).  Same
    bits as the aligned run and the oracle; nothing written past either end
    of the output views (checked in run_sorted)."""
    name = "align-n%d" % n
    gi, gp = check_sorted_case(dev, name, 1, off)
    ai, ap = check_sorted_case(dev, name, 1)
    assert_ids(gi, ai)
    assert_bits(gp, ap)


# ---------------------------------------------- 5. explicit-index kernels
def run_local(dev, tp, tn, tc, tcn, ti, n, m, u, kmajor, relative):
    import torch
    from pcr_amd import _lib
    from pcr_amd.ops import _ptr, _stream
    b = tp.shape[0]
    nan = float("nan")
    bo, out = guarded(dev, (b, 4, u, m), torch.float32, nan)
    _lib.check(_lib.load().pcr_local_ppf_forward(
        _ptr(tp), _ptr(tn), _ptr(tc), _ptr(tcn), _ptr(ti), b, n, m, u, int(kmajor), int(relative),
        _ptr(out), _stream()), "local_ppf_forward")
    torch.cuda.synchronize()
    assert guards_intact(bo, out, nan), "local PPF written outside its output"
    return N(out)


@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("kmajor", [True, False])
@pytest.mark.parametrize("n,m,u", R.LOCAL_SHAPES)
def test_local_ppf_forward_tails_and_bad_ids(dev, n, m, u, kmajor, relative):
    """pcr_local_ppf_forward with point tails (300, 2049, 257, 700), slot
    tails (u = 13, 9, 20), n != m, both id layouts and ids of -1, n, n + 5,
    INT_MAX, INT_MIN and a whole row of -1.  Centres that are the points'
    own tensors take local_ppf_self_kernel<8> (k-major, n <= 2048); cloned
    centres take local_ppf_kernel: both must give the oracle's bits."""
    pts, nrm, ctr, cnrm, ids = R.local_case(n, m, u, kmajor)
    exp = R.local_expected(n, m, u, kmajor, relative)
    tp, tn, ti = T(pts, dev), T(nrm, dev), T(ids, dev)
    if n == m:
        same = run_local(dev, tp, tn, tp, tn, ti, n, m, u, kmajor, relative)
        assert_bits(same, exp, "ppf (centres are the points)")
        tc, tcn = tp.clone(), tn.clone()
        assert tc.data_ptr() != tp.data_ptr() and tcn.data_ptr() != tn.data_ptr()
    else:
        tc, tcn = T(ctr, dev), T(cnrm, dev)
    got = run_local(dev, tp, tn, tc, tcn, ti, n, m, u, kmajor, relative)
    assert_bits(got, exp, "ppf (separate centres)")
    ref = R.local_ppf_f64(pts, nrm, ctr, cnrm, ids, kmajor, relative)
    R.compare_local(got, ref, R.unit_rows(nrm), R.unit_rows(cnrm), ids, kmajor)


# -------------------------------------------------------- 5. global PPF
@pytest.mark.parametrize("n", R.GLOBAL_SIZES)
def test_spherical_ppf_forward_thresholds(dev, n):
    """global_ppf_kernel at n = 1, 255, 257, 1000 with normals of length
    0.9e-10 / 1.1e-10 (either normal), a point on and 1e-30 from its centre,
    NaN inputs and normals of length 1e-5 / 1e5."""
    import torch
    from pcr_amd import _lib
    from pcr_amd.ops import _ptr, _stream
    xyz, ctr, nrm, cnrm, exp, _ = R.global_case(n)
    nan = float("nan")
    bf, feat = guarded(dev, exp.shape, torch.float32, nan)
    tx, tc, tn, tcn = (T(a, dev) for a in (xyz, ctr, nrm, cnrm))
    _lib.check(_lib.load().pcr_spherical_ppf_forward(
        _ptr(tx), _ptr(tc), _ptr(tn), _ptr(tcn), exp.shape[0], n, _ptr(feat), _stream()),
        "spherical_ppf_forward")
    torch.cuda.synchronize()
    assert guards_intact(bf, feat, nan)
    got = N(feat)
    assert_bits(got, exp, "global ppf")
    R.compare_global(got, *R.global_ppf_f64(xyz, ctr, nrm, cnrm))
