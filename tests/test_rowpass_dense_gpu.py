"""GPU: the row-pass kernels -- forward P~ = K^ C with its fused row statistics, the weighted Gram H = K^T diag(beta) K^, colstats, the
fold-pair forward -- element by element against the extended-precision reference of tests/rowpass_ref.py on DENSE, well-conditioned
operands: every Gram tile, every k-step of the forward and every column group carries numbers an indexing error would
move far beyond the bound

    |got - R| <= C_KERNEL[kind] * 2^-52 * S      per element, S = the element's own condition scale (never an array maximum).

What is read: the statistic bundle between hmogp_step_begin and hmogp_step_finish (lower triangle of H), dL_dKmn / dL_dKdiag of the
inner-protocol export, and q(f) through hmogp_predict_f (the triangular fold; it uses the factorisation of the evaluation it follows,
forced rung included).  Every test prints its worst ratios as `[rowpass] <case> <kind> ...`.

Cases G, H, I take the regular kernels to 3-D and 4-D inputs and to HMOGP_MAXQ latents (`rbf_kernel<3|4>`, `colstats_kernel<3|4, ...>`,
`window_kernel<3>`, `strict_rowstats_kernel<3|4>`, the row pass batched over eight latents); they are held to C_KERNEL_WIDE."""
import numpy as np
import pytest

import rowpass_cases as rc
import rowpass_ref as rr

pytestmark = pytest.mark.gpu

_CASES = {}


@pytest.fixture(scope="module")
def refs():
    return rc.references()


def case(tag):
    if tag not in _CASES:
        _CASES[tag] = rc.dense_case(tag)
    return _CASES[tag]


def engine(tag, **kw):
    from hetmogp_amd.engine import Engine
    prm, prob, X, Y, _ = case(tag)
    e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
    e.set_data(X, Y)
    return e


def evaluate(e, tag, fused=False, raw=True, predict=True, **kw):
    """One evaluation at the forced rung -> everything the criterion compares, as a dict kind -> array(s).
    fused=False: hmogp_step_begin, the bundle, hmogp_step_finish (the split step always takes the regular kernels);
    fused=True: hmogp_elbo_grad, then the bundle it left (the only way onto the fused small-model kernels)."""
    prm, prob, X, Y, rungs = case(tag)
    T, Q, Df = prob["T"], prob["Q"], prob["Df"]
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"], forced_rung=rungs)
    args.update(kw)
    if fused:
        out = e.elbo_grad(**args)
        stats = e.stats_read()
    else:
        e.step_begin(**args)
        stats = e.stats_read()
        out = e.step_finish()
    assert out["rungs"] == rungs and not out["v_negative"]
    got = rr.split_bundle(stats, prob)
    b = kw.get("row_begin") or [0] * T
    en = kw.get("row_end") or [x.shape[0] for x in X]
    if raw:
        g = e.debug_raw_grads([en[t] - b[t] for t in range(T)])
        got["dKmn"], got["dKdiag"] = g["dL_dKmn"], g["dL_dKdiag"]
    if predict:
        got["m"], got["v"] = [None] * Df, [None] * Df
        for t in range(T):
            m, v = e.predict_f(X[t][b[t]:en[t]])
            for d in range(Df):
                if prob["f_index"][d] == t:
                    got["m"][d], got["v"][d] = m[:, d].copy(), v[:, d].copy()
    return got


def ck(tag):
    """Cases A-F: C_KERNEL; cases G, H, I: C_KERNEL_WIDE (the same rule over their own oracle measurement)."""
    return rr.c_kernel_wide() if tag in rc.WIDE_TAGS else rr.c_kernel()


def same_bits(a, b, kinds):
    for k in kinds:
        for (label, x, _, _), (_, y, _, _) in zip(rr.pairs(k, a[k], a[k], a[k]), rr.pairs(k, b[k], b[k], b[k])):
            assert np.array_equal(np.asarray(x), np.asarray(y)), ("not bit-identical", k, label)


@pytest.mark.parametrize("tag", sorted(rc.CASES))
def test_dense_case_vs_extended_precision(refs, tag):
    """Cases A-I on the default engine through the split step: the bundle, the inner-protocol gradients and q(f), every element; a second
    identical evaluation gives the same bits."""
    R, S = refs[tag]["default"]
    e = engine(tag)
    got = evaluate(e, tag)
    rr.check(tag, got, R, S, ck(tag), rr.KINDS)
    same_bits(got, evaluate(e, tag), rr.KINDS)
    e.close()


@pytest.mark.parametrize("small_path", [True, False])
def test_case_A_fused_small_model_kernels_and_regular_kernels(refs, small_path):
    """M = 64 through hmogp_elbo_grad: the fused small-model kernels (small_path=True) and the regular kernels in their place."""
    R, S = refs["A"]["default"]
    e = engine("A", small_path=small_path)
    got = evaluate(e, "A", fused=True)
    rr.check("A fused small_path=%s" % small_path, got, R, S, rr.c_kernel(), rr.KINDS)
    same_bits(got, evaluate(e, "A", fused=True), rr.KINDS)
    e.close()


def test_case_C_exact_zero_windows_cover_everything(refs):
    """Nothing is exactly zero on dense operands: the windows must cover every tile and give the dense result under the same constants
    (the windows split the rows into ranges of their own: the inner-protocol export, which needs one pool, is left out)."""
    R, S = refs["C"]["default"]
    e = engine("C", exact_zero_windows=True)
    rr.check("C exact_zero_windows", evaluate(e, "C", raw=False), R, S, rr.c_kernel(), rr.BUNDLE_KINDS + ("m", "v"))
    e.close()


def test_case_D_row_pools_of_300(refs):
    """chunk_rows = 300: several pools, tasks cut into segments (the inner-protocol export needs one pool and is left out)."""
    R, S = refs["D"]["default"]
    e = engine("D", chunk_rows=300)
    kinds = rr.BUNDLE_KINDS + ("m", "v")
    got = evaluate(e, "D", raw=False)
    rr.check("D chunk_rows=300", got, R, S, rr.c_kernel(), kinds)
    same_bits(got, evaluate(e, "D", raw=False), kinds)
    e.close()


@pytest.mark.parametrize("mask", ["GROUP_QU", "GROUP_HYPER"])
def test_case_D_group_masks(refs, mask):
    """E-steps (group QU: the fold-pair forward, P~ never stored) and hyper-parameter steps: ve, sgv, H, r of the bundle."""
    from hetmogp_amd import _lib
    R, S = refs["D"]["default"]
    e = engine("D")
    got = evaluate(e, "D", raw=False, predict=False, group_mask=getattr(_lib, mask))
    rr.check("D " + mask, got, R, S, rr.c_kernel(), ("ve", "sgv", "H", "r"))
    e.close()


def test_case_D_batch_scale(refs):
    R, S = refs["D"]["bs"]
    e = engine("D")
    rr.check("D batch_scale", evaluate(e, "D", batch_scale=rc.D_BATCH_SCALE), R, S, rr.c_kernel(), rr.KINDS)
    e.close()


def test_case_D_row_shard_off_the_16_row_grid(refs):
    """A row shard [row_begin, row_end) whose first rows are no multiples of 16, against the reference of those rows."""
    R, S = refs["D"]["shard"]
    e = engine("D")
    got = evaluate(e, "D", row_begin=list(rc.D_SHARD[0]), row_end=list(rc.D_SHARD[1]))
    rr.check("D row shard", got, R, S, rr.c_kernel(), rr.KINDS)
    e.close()


def test_case_D_strict_one_solve_form(refs):
    """strict_qf=True: the bundle's H and r hold X^T diag(beta) X and X^T alpha with X = K^ Luu^-T; the rest is the same mathematics."""
    R, S = refs["D"]["strict"]
    e = engine("D", strict_qf=True)
    got = evaluate(e, "D", raw=False, predict=False)
    rr.check("D strict_qf", got, R, S, rr.c_kernel(), rr.BUNDLE_KINDS)
    e.close()


# ------------------------------------------------------------------------------------------------ 3-D / 4-D inputs, eight latents
def test_case_I_row_pools_of_100(refs):
    """Eight latents with chunk_rows = 100: several pools, tasks cut into segments, the batched row pass once per pool."""
    R, S = refs["I"]["default"]
    e = engine("I", chunk_rows=100)
    kinds = rr.BUNDLE_KINDS + ("m", "v")
    got = evaluate(e, "I", raw=False)
    rr.check("I chunk_rows=100", got, R, S, ck("I"), kinds)
    same_bits(got, evaluate(e, "I", raw=False), kinds)
    e.close()


@pytest.mark.parametrize("tag", ["G", "H"])
def test_cases_G_H_strict_one_solve_form(refs, tag):
    """strict_qf=True at P = 3 and P = 4: `strict_rowstats_kernel<P>` and `colstats_kernel<P, true, ...>`."""
    R, S = refs[tag]["strict"]
    e = engine(tag, strict_qf=True)
    rr.check(tag + " strict_qf", evaluate(e, tag, raw=False, predict=False), R, S, ck(tag), rr.BUNDLE_KINDS)
    e.close()


def test_case_H_row_shard_off_the_16_row_grid(refs):
    """P = 4 and a row shard whose first rows are no multiples of 16: the X offset of a task is row_begin * 4 doubles."""
    R, S = refs["H"]["shard"]
    e = engine("H")
    got = evaluate(e, "H", row_begin=list(rc.H_SHARD[0]), row_end=list(rc.H_SHARD[1]))
    rr.check("H row shard", got, R, S, ck("H"), rr.KINDS)
    e.close()


def test_case_G_exact_zero_windows_cover_everything(refs):
    """Exact-zero windows asked for explicitly at P = 3 (`window_kernel<3>`, `colstats_kernel<3, ., ., true>`): nothing is exactly
    zero, the windows must cover every tile (their row ranges refuse the inner-protocol export, which is left out)."""
    R, S = refs["G"]["default"]
    e = engine("G", exact_zero_windows=True)
    rr.check("G exact_zero_windows", evaluate(e, "G", raw=False), R, S, ck("G"), rr.BUNDLE_KINDS + ("m", "v"))
    e.close()


def test_case_G_row_weights_follow_the_evaluation(refs):
    """Three evaluations on one engine: default, batch_scale = [1, 3.5, 0.25], default again.  The row-weight buffers keep their
    addresses from one evaluation to the next: `colstats_kernel<3, ., ., false>` reads alpha, alpha0, beta0 through the constant address
    space and must see the values of the CURRENT evaluation."""
    e = engine("G")
    first = evaluate(e, "G")
    rr.check("G first", first, *refs["G"]["default"], ck("G"), rr.KINDS)
    rr.check("G then batch_scale", evaluate(e, "G", batch_scale=rc.D_BATCH_SCALE), *refs["G"]["bs"], ck("G"), rr.KINDS)
    same_bits(first, evaluate(e, "G"), rr.KINDS)
    e.close()
