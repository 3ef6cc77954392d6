"""The PPF oracle (include/pcr_math.h through oracle/) against the independent
float64 restatement of tests/ppf_restate.py on every input family of
test_gpu_ppf.py, and the properties of those inputs the GPU tests rely on
(shares of pairs off the shared-reciprocal path, cosines on both sides of the
acos seam, unfilled slots, planted rows), so that an edit to a generator
cannot quietly empty a case.  No GPU."""
import numpy as np
import pytest

import oracle
import ppf_restate as R

NORMAL_CASES = ["normals-n%d" % n for n in R.NORMAL_SIZES]


# ------------------------------------------------ the references themselves
def test_local_ppf_f64_known_answers():
    """One centre at (1, 0, 0) with normal +y, neighbours at the origin
    (normal +x), at (1, 1, 0) (normal +y) and the centre itself."""
    pts = np.array([[[0.0, 1.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]])
    nrm = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 0.0, 0.0]]])
    ctr, cn = pts[:, :, 2:], nrm[:, :, 2:]
    idx = np.array([[[0], [1], [2], [-1], [3]]], np.int32)  # k-major [1, 5, 1]
    r1 = R.local_ppf_f64(pts, nrm, ctr, cn, idx, True, 1)[0, :, :, 0]
    r0 = R.local_ppf_f64(pts, nrm, ctr, cn, idx, True, 0)[0, :, :, 0]
    # d = 2c - p: (2, 0, 0), (1, -1, 0), (1, 0, 0); -1 and 3 read neighbour 0
    s = np.sqrt(0.5)
    assert np.allclose(r1, [[1, -s, 0, 1, 1], [0, -s, 0, 0, 0], [0, 1, 1, 0, 0],
                            [2, np.sqrt(2), 1, 2, 2]], atol=1e-15)
    # d = c - p: (1, 0, 0), (0, -1, 0), 0 (undefined direction)
    assert np.allclose(r0[:, [0, 1, 3, 4]], [[1, -1, 1, 1], [0, -1, 0, 0], [0, 1, 0, 0],
                                             [1, 1, 1, 1]], atol=1e-15)
    assert np.isnan(r0[:2, 2]).all() and r0[2, 2] == 1 and r0[3, 2] == 0
    rm = R.local_ppf_f64(pts, nrm, ctr, cn, np.ascontiguousarray(idx.transpose(0, 2, 1)), False, 1)
    assert np.array_equal(rm[0, :, :, 0], r1)


def test_global_ppf_f64_known_answers():
    xyz = np.array([[[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]])
    ctr = np.array([[[3.0, 1.0, 1.0, 0.0], [4.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]])
    nrm = np.array([[[2.0, 1.0, 0.0, 1e-10], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])
    cn = np.array([[[0.0, 0.0, 0.0, 0.0], [0.5, 1.0, 1.0, 1.0], [0.0, 0.0, np.nan, 0.0]]])
    ref, zero = R.global_ppf_f64(xyz, ctr, nrm, cn)
    assert zero.tolist() == [[False, False, False, True]]
    assert np.allclose(ref[0, :, 0], [0.8, 0.6, 0.0, 5.0], atol=1e-15)
    assert np.allclose(ref[0, :, 1], [0.0, 0.0, 0.0, 1e-20], atol=1e-30)  # point on its centre
    assert np.allclose(ref[0, :, 2], [1.0, 0.0, 1.0, 1.0], atol=1e-15)  # NaN normal reads as 1
    assert (ref[0, :, 3] == 0).all()


# ------------------------------------------------------------ sorted path
ALIGN_CASES = ["align-n1024", "align-n516"]
# Gaussian clouds at the small scales: the only cases with out-of-range pairs
SMALL_SCALE = ("e-61", "e-60", "e-59")


@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("name", R.SCALE_CASES + R.SIZE_CASES + ALIGN_CASES + NORMAL_CASES)
def test_sorted_case_oracle_vs_f64(name, relative):
    """Cosines within 2e-6 and |d| within 1e-6 relative where the normals are
    unit; NaN exactly where float64 is undefined.  Per cloud: the undefined
    share under its cap (and, with relative = 0, at least the self pair's
    1 / k); the out-of-range share (fp32 cannot hold |d|^2, see
    ppf_restate.DN_LO) 0 except on the Gaussian clouds at 2^-61 .. 2^-59, and
    capped there; every channel bounded on all its eligible elements less the
    capped shares (check_sorted_case_f64).

    Measured on the out-of-range pairs (|d| < 2^-64), where the oracle itself
    leaves the bounds: at 2^-61 up to 378 of a case's 65536 pairs (0.6%), off
    by up to 1.4e-5 relative on |d| and 6.9e-6 on the cosines; at 2^-60 up to
    38 pairs (0.06%), 2.7e-6 and 2.2e-6; at 2^-59 up to 4 pairs, inside the
    bounds.  Everywhere else the worst is 3.2e-7 / 3.0e-7."""
    fig = R.check_sorted_case_f64(name, relative)
    _, _, k, _, _ = R.sorted_case(name, relative)
    print("%s relative=%d: excluded %s (cap %s), out of range %s (cap %.5f), cos %.3g, |d| %.3g, "
          "bounded %s of %s" % (name, relative, fig["excluded"], fig["excluded_cap"],
                                fig["out_of_range"], fig["range_cap"], fig["cos"], fig["dn"],
                                fig["bounded"].tolist(), fig["eligible"].tolist()))
    if not (name[0] == "A" and name.endswith(SMALL_SCALE)):
        assert fig["range_cap"] == 0 and (fig["out_of_range"] == 0).all()
    assert fig["range_cap"] <= 0.02
    if not relative:
        assert (fig["excluded"] >= 1.0 / k - 1e-12).all()
    # the d-dependent channels are compared on every cloud with unit normals
    unit_clouds = R.unit_rows(R.sorted_case(name, relative)[1]).mean(axis=1) >= 0.98
    assert unit_clouds.any()
    floor = (1.0 - fig["excluded_cap"] - fig["range_cap"] - 0.06) * fig["pairs"]
    assert (fig["bounded"][unit_clouds] >= floor[unit_clouds, None]).all()


# family B's shares of pairs off the shared-reciprocal path, relative = 1
B_UNSAFE = {-61: 1.0, -60: 0.905, -59: 0.495, 0: 0.001, 58: 0.014, 59: 0.64, 60: 0.94}


@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("name", R.SCALE_CASES)
def test_scale_case_mixes_safe_and_unsafe_pairs(name, relative):
    xyz, _, k, ids, _ = R.sorted_case(name, relative)
    share = float(R.unsafe_pairs(xyz, ids, relative).mean())
    e = int(name.rsplit("e", 1)[1]) if name != "C" else None
    print("%s relative=%d: unsafe share %.4f" % (name, relative, share))
    if name.startswith("B") and relative:
        assert abs(share - B_UNSAFE[e]) <= 0.005
    if e == -61:
        assert share >= 0.99
    elif e == 0:
        assert share <= 0.01 + (0 if relative else 0.06)  # the self pair and duplicates
    elif e == -60 and not relative:
        assert share >= 0.99  # neighbour distances of ~0.1 * 2^-60: (nearly) all unsafe
    else:
        # safe and unsafe lanes share every 64-pair wave
        assert 0.01 <= share <= 0.99
    if not relative:
        assert share >= 1.0 / k
    if e is not None and e >= 40:
        # every neighbour lies past the KNN's cut-off: slot 0 is the point, the rest read 0
        # (the lattice's duplicates still find each other)
        assert (ids[:, 1:] == 0).mean() >= (1.0 if name[0] == "A" else 0.95)
        if name[0] == "A":
            assert (ids[:, 0] == np.arange(xyz.shape[2])).all()
    if e == -61 and name[0] == "B":
        d, _ = oracle.knn_dir(xyz, xyz, k)
        assert d[d > 0].min() >= np.float32(2.0 ** -126)  # nothing in the KNN is denormal


def test_family_c_cluster_is_its_own_neighbourhood():
    xyz, _, _, ids, _ = R.sorted_case("C", 1)
    assert (ids[:, :, :64] < 64).all()
    us = R.unsafe_pairs(xyz, ids, 1)
    assert us[:, :, :64].mean() >= 0.5 and not us[:, :, 64:].any()
    assert not us[:, :, :64].all()


# ------------------------------------------------- normals and the acos seam
@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("name", NORMAL_CASES)
def test_normals_case_properties(name, relative):
    xyz, nrm, k, ids, ppf = R.sorted_case(name, relative)
    unit = R.unit_rows(nrm)
    n = xyz.shape[2]
    assert unit[0].all() and not unit[2].any()
    assert unit[1].sum() == n - 14  # zero, NaN, inf, tiny and huge rows
    ref = R.local_ppf_f64(xyz, nrm, xyz, nrm, ids, True, relative)
    # planted centre normals: slot 1's cosine with d at +-1 and at the +-0.5 seam
    s = R.PLANT["seam"]
    got = ref[1, 1, 1, s]
    assert np.abs(got - np.repeat(R.SEAM_COS, 8)).max() <= 1e-7
    ang = ppf[1, 1, 1, s].astype(np.float64)
    assert np.abs(np.cos(ang) - np.repeat(R.SEAM_COS, 8)).max() <= R.COS_TOL
    # both acos ranges and both tails on the unit clouds; heavy clamping on cloud 2
    for b in (0, 1):
        c = ref[b, :3][np.isfinite(ref[b, :3])]
        assert (np.abs(c) <= 0.5).mean() >= 0.3
        assert (c > 0.5).mean() >= 0.1 and (c < -0.5).mean() >= 0.1
    assert (np.abs(ref[2, :3]) == 1.0).mean() >= 0.25
    assert (np.abs(ref[0, :3]) == 1.0).mean() <= 0.02  # the self pair's normal . normal
    # the non-finite rows reach the output
    assert np.isnan(ppf[1, 1, :, R.PLANT["nan"]]).all()
    assert np.isnan(ppf[1]).sum() > np.isnan(ppf[0]).sum()


# ------------------------------------------------------------ dispatch lines
@pytest.mark.parametrize("name", R.SIZE_CASES)
def test_size_case_properties(name):
    xyz, nrm, k, ids, _ = R.sorted_case(name, 1)
    n = xyz.shape[2]
    d, _ = oracle.knn_dir(xyz, xyz, k)
    if n < k:
        # slots n .. k - 1 are unfilled: (10000, 0)
        assert (d[:, n:] == 10000).all() and (ids[:, n:] == 0).all()
        assert (d[:, :n] < 10000).all()
    else:
        assert (d < 10000).all()
    assert R.unit_rows(nrm).all()
    assert name in R.SORTED_CASES and (ids[:, 0] == np.arange(n)).all()


def test_size_cases_cover_the_dispatch_lines():
    names = set(R.SIZE_CASES)
    for n in (4, 5, 512, 513, 516, 1020, 1028, 2045, 2048):
        for k in (32, 31):
            assert "size-n%d-k%d" % (n, k) in names
    assert "size-b3-n516-k7" in names
    # 3 clouds x 4 slot groups x 2 point ranges: a multiple of 8 workgroups whose
    # per-cloud share (8) is not what the XCD remap deals per XCD (3)
    xyz, _, k, _, _ = R.sorted_case("size-b3-n516-k7", 1)
    units = xyz.shape[0] * ((k + 1) // 2) * 2
    assert units % 8 == 0 and (units // xyz.shape[0]) != units // 8


# ------------------------------------------------------- explicit indices
@pytest.mark.parametrize("relative", [1, 0])
@pytest.mark.parametrize("kmajor", [True, False])
@pytest.mark.parametrize("n,m,u", R.LOCAL_SHAPES)
def test_local_case_oracle_vs_f64(n, m, u, kmajor, relative):
    pts, nrm, ctr, cnrm, ids = R.local_case(n, m, u, kmajor)
    out = R.local_expected(n, m, u, kmajor, relative)
    ref = R.local_ppf_f64(pts, nrm, ctr, cnrm, ids, kmajor, relative)
    fig = R.compare_local(out, ref, R.unit_rows(nrm), R.unit_rows(cnrm), ids, kmajor)
    print("(%d, %d, %d) kmajor=%d relative=%d: excluded %s, cos %.3g, |d| %.3g, bounded %s"
          % (n, m, u, kmajor, relative, fig["excluded"], fig["cos"], fig["dn"],
             fig["bounded"].tolist()))
    assert (fig["out_of_range"] == 0).all() and (fig["eligible"] == fig["pairs"]).all()
    if relative or n != m:
        cap = 0.0
    else:
        cap = 1.0 / u + 0.01  # the self pair; the planted ids and row move a few
        assert (fig["excluded"] > 0.5 / u).all()
    R.assert_coverage(fig, cap, 0.0)
    # the planted ids are there, in this layout
    km = ids if kmajor else ids.transpose(0, 2, 1)
    assert km.shape == (2, u, m)
    for b in range(2):
        assert km[b, 0, :5].tolist() == [-1, n, n + 5, 2 ** 31 - 1, -2 ** 31]
        assert (km[b, :, 7 + 100 * b] == -1).all() and km[b, u - 1, m - 1] == n
    assert ((km >= 0) & (km < n)).mean() >= 0.99


# ------------------------------------------------------------- global PPF
@pytest.mark.parametrize("n", R.GLOBAL_SIZES)
def test_global_case_oracle_vs_f64(n):
    xyz, ctr, nrm, cnrm, out, col = R.global_case(n)
    ref, zero = R.global_ppf_f64(xyz, ctr, nrm, cnrm)
    cmax, dmax, count = R.compare_global(out, ref, zero)
    print("n=%d: cos %.3g, |d| %.3g over %d" % (n, cmax, dmax, count))
    if n == 1:
        assert not zero.any() and count == out.size
        return
    assert set(col) == set(R.G_PLANT) and len(set(col.values())) == len(col)
    z = np.zeros(n, bool)
    z[[col["n_below"], col["cn_below"]]] = True
    assert (zero == z).all()  # 0.9e-10 is the zero row, 1.1e-10 is not
    for name in ("n_above", "cn_above", "short", "long"):
        assert (out[:, 3, col[name]] > 0.01).all()
    for name in ("coincide", "near", "nan_xyz"):
        assert (out[:, 3, col[name]] == np.float32(1e-20)).all()  # the 1e-20 clamp
    assert (ref[:, :2, col["coincide"]] == 0).all()
    assert (np.abs(ref[:, :2, col["near"]]) > 0).all()  # 1e-30 / 1e-20, not 0
    assert (out[:, :2, col["nan_xyz"]] == 0).all() and (out[:, 0, col["nan_nrm"]] == 0).all()
    assert count == out.size - 4 * zero.sum()
