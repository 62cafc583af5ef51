"""GPU: the gradient tail -- everything between the statistic bundle and the numbers the optimiser consumes -- element by element
against the extended-precision reference of tests/tail_ref.py.  Pinned: the M x M products with their special modes
(`lower_only` + mirror for G, the `a_tri` / `b_tri` k-range trims of S = L L^T and dL_dS L, the transposed form K^-1 S G,
`gemm_small_kernel` against `gemm_f64_kernel` on ragged M), `gemv_kernel`, `dlds_kernel`, `pack_gl_kernel`, `gmu_kernel`,
`dkmm_tiled_kernel`, `kzz_rows_kernel<P>`, `kl_terms_kernel`, `tri_fold_kernel` / `sub_kernel` (C, `posterior_u`),
`gather_small_kernel`, the host assembly of `finish_tail`, and for M <= 64 the fused `u_small_kernel` / `finish_small_kernel`.

    |got - R| <= C_KERNEL[kind] * 2^-52 * S      per element, S = the element's own running error bound (never an array maximum).

Cases (a), (b) of tests/tail_cases.py inject a float64 bundle taken as exact between `step_begin` and `step_finish`; cases (c) run end
to end through `hmogp_elbo_grad` and add the bundle's own 9c bound pushed through the tail.  Every test prints its worst ratios as
`[tail] <case> <kind> ...`."""
import numpy as np
import pytest

import rowpass_cases as rc
import rowpass_ref as rr
import tail_cases as tc
import tail_ref as tr

pytestmark = pytest.mark.gpu

ALL_TAGS = rc.BASE_TAGS + list(tc.TAIL_ONLY)
VARIANTS = [(t, "default") for t in ALL_TAGS] + [("D", "bs"), ("D", "strict")]
OUT_KINDS = tuple(k for k in tr.KINDS if k not in ("wv", "winv"))


@pytest.fixture(scope="module")
def refs():
    return tc.references()


def make_engine(case, **kw):
    from hetmogp_amd.engine import Engine
    prm, prob, X, Y, _ = case
    e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
    e.set_data(X, Y)
    return e


def params(case, **kw):
    prm, _, _, _, rungs = case
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"], forced_rung=rungs)
    args.update(kw)
    return args


def collect(e, out, case, want_dL_dS=True):
    assert out["rungs"] == case[4]
    wv, winv = e.posterior_u()
    got = {k: np.array(out[k], dtype=np.float64, copy=True) for k in OUT_KINDS if k not in ("elbo", "dL_dS")}
    got["elbo"] = np.array([out["elbo"]])
    if want_dL_dS:
        got["dL_dS"] = np.array(out["dL_dS"], copy=True)
    got["wv"], got["winv"] = wv, winv
    return got


def split_step(e, case, bundle, **kw):
    """hmogp_step_begin (the u-side chain; its own row pass fills the bundle) -> the injected bundle -> hmogp_step_finish with dL_dS ->
    hmogp_posterior_u."""
    e.step_begin(**params(case, **kw))
    e.stats_write(np.asarray(bundle, dtype=np.float64))
    return collect(e, e.step_finish(want_dL_dS=True), case)


def same_bits(a, b, kinds=tr.KINDS):
    for k in kinds:
        assert np.array_equal(a[k], b[k]), ("not bit-identical", k)


@pytest.mark.parametrize("tag,variant", VARIANTS)
def test_tail_vs_extended_precision(refs, tag, variant):
    """Cases (a) and (b): every kind, every element within C_KERNEL; a second identical evaluation gives the same bits."""
    o, case = refs[tag][variant], refs[tag]["case"]
    e = make_engine(case, strict_qf=True) if o["strict"] else make_engine(case)
    try:
        got = split_step(e, case, o["bundle"])
        tr.check("%s %s" % (tag, variant), got, o["R"], o["S"], tr.c_kernel())
        same_bits(got, split_step(e, case, o["bundle"]))
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["GROUP_QU", "GROUP_HYPER", "skip_g_L"])
def test_case_D_group_masks_and_skip_g_L(refs, mode):
    """The computed groups are held to the same bound, the others are exactly 0.0."""
    from hetmogp_amd import _lib
    o, case = refs["D"]["default"], refs["D"]["case"]
    zero = dict(GROUP_QU=("g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"), GROUP_HYPER=("g_m_u", "g_L_u", "g_Z"),
                skip_g_L=("g_L_u",))[mode]
    kw = dict(skip_g_L=True) if mode == "skip_g_L" else dict(group_mask=getattr(_lib, mode))
    e = make_engine(case)
    try:
        got = split_step(e, case, o["bundle"], **kw)
        for k in zero:
            assert np.all(got[k] == 0.0) and not np.any(np.signbit(got[k])), (mode, k, "not exactly 0.0")
        tr.check("D " + mode, got, o["R"], o["S"], tr.c_kernel(), tuple(k for k in tr.KINDS if k not in zero))
    finally:
        e.close()


@pytest.mark.parametrize("small_path", [True, False])
@pytest.mark.parametrize("tag", list(tc.SMALL))
def test_small_model_shapes_end_to_end(refs, tag, small_path):
    """Cases (c): M = 33, 50, 64 through hmogp_elbo_grad on the fused small-model kernels (witness: only that path captures a hipGraph)
    and on the regular kernels; bound 2^-52 (C_KERNEL S_tail + B), B = the bundle's own 9c bound pushed through the tail."""
    o, case = refs[tag]["default"], refs[tag]["case"]
    e = make_engine(case, small_path=small_path)
    try:
        for _ in range(3):
            out = e.elbo_grad(**params(case))
        replayed = collect(e, out, case, want_dL_dS=False)
        stats = e.graph_stats()
        assert (stats[0] >= 1) if small_path else (stats == (0, 0)), stats
        what = "%s small_path=%s" % (tag, small_path)
        tr.check(what + " (3rd call)", replayed, o["R"], o["S"], tr.c_kernel(), tuple(k for k in tr.KINDS if k != "dL_dS"), B=o["B"])
        got = collect(e, e.elbo_grad(want_dL_dS=True, **params(case)), case)
        tr.check(what + " (with dL_dS)", got, o["R"], o["S"], tr.c_kernel(), B=o["B"])
    finally:
        e.close()


def numpy_wire(bundle, prob):
    """The wire format restated: head | per latent the lower triangle of H_q in row-major order, then r, dZ, sa, sl, swk."""
    lay, M = rr.layout(prob), prob["M"]
    parts = [bundle[:lay["NG"]]]
    for q in range(prob["Q"]):
        b = bundle[lay["NG"] + q * lay["per_q"]:lay["NG"] + (q + 1) * lay["per_q"]]
        parts += [b[:M * M].reshape(M, M)[np.tril_indices(M)], b[M * M:]]
    return np.concatenate(parts)


@pytest.mark.parametrize("tag", ["B", "D", "T330"])
def test_seams_of_the_bundle(refs, tag):
    """The bundle's ways in and out, bit for bit, on a bundle whose UPPER triangles hold other numbers than the lower ones (the engine
    reads the lower triangle; a transposed wire triangle is invisible on a symmetric or banded H): stats_write(stats_read()) changes
    nothing; the junk upper triangle changes nothing; wire_pack -> wire_read is the NumPy packing; wire_write -> wire_unpack ->
    stats_read restores every lower triangle and everything outside H."""
    o, case = refs[tag]["default"], refs[tag]["case"]
    prob = case[1]
    lay, M, Q = rr.layout(prob), prob["M"], prob["Q"]
    bundle = np.asarray(o["bundle"], dtype=np.float64)
    junk = bundle.copy()
    rng = np.random.RandomState(77)
    up = np.triu_indices(M, 1)
    for q in range(Q):
        H = junk[lay["NG"] + q * lay["per_q"]:][:M * M].reshape(M, M)
        H[up] = rng.randn(up[0].size)
    e = make_engine(case)
    try:
        plain = split_step(e, case, bundle)
        same_bits(plain, split_step(e, case, junk))
        e.step_begin(**params(case))
        e.stats_write(junk)
        back = e.stats_read()
        assert np.array_equal(back, junk)
        e.wire_pack()
        wire = e.wire_read()
        assert np.array_equal(wire, numpy_wire(junk, prob))
        e.stats_write(np.zeros_like(junk))
        e.wire_write(wire)
        e.wire_unpack()
        restored = e.stats_read()
        lo = np.tril(np.ones((M, M), dtype=bool))
        assert np.array_equal(restored[:lay["NG"]], junk[:lay["NG"]])
        for q in range(Q):
            a = restored[lay["NG"] + q * lay["per_q"]:lay["NG"] + (q + 1) * lay["per_q"]]
            b = junk[lay["NG"] + q * lay["per_q"]:lay["NG"] + (q + 1) * lay["per_q"]]
            assert np.array_equal(a[:M * M].reshape(M, M)[lo], b[:M * M].reshape(M, M)[lo]), (q, "lower triangle of H")
            assert np.array_equal(a[M * M:], b[M * M:]), (q, "r, dZ, sa, sl, swk")
        e.stats_write(back)
        same_bits(plain, collect(e, e.step_finish(want_dL_dS=True), case))
    finally:
        e.close()
