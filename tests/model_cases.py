"""The whole-model harness of the GPU suite: the seeded case generator, the engine helpers, and the three checks every likelihood
family added after the reference's eight runs against the oracle (one row pool / several / minibatch, small-model path against the
regular one, strict q(f) against the literal oracle).  A plain module: seeds, shapes and spec sets stay in the test files.

Yardstick of every oracle comparison here: conftest.assert_parity with its own constants (array-normalised 1e-8 and element-wise
1e-5 relative with floor 1e-9)."""
import numpy as np

from conftest import assert_parity, elementwise_excess, rel_norm

KEYS = ["elbo", "g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"]


def make_engine(prob, X, Y, **kw):
    from hetmogp_amd.engine import Engine
    e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
    e.set_data(X, Y)
    return e


def run(e, prm, bs=None, **kw):
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"],
                lengthscale=prm["lengthscale"], W=prm["W"], kappa=prm["kappa"], W0=prm.get("W0"), batch_scale=bs)
    args.update(kw)
    return e.elbo_grad(**args)


def synth(seed, specs, Ns, M, Q, P, cs):
    """Seeded synthetic case in the style of the fixtures (oracle/make_golden.py:build_case)."""
    from oracle import svmogp_oracle as so
    rng = np.random.RandomState(seed)
    prob = so.make_problem(specs, Q, M, P)
    Df = prob["Df"]
    X = [np.sort(rng.rand(n, P), axis=0) if P == 1 else rng.rand(n, P) for n in Ns]
    Y = []
    for (name, kw), n in zip(specs, Ns):
        if name in ("Gaussian", "HetGaussian"):
            Y.append(rng.randn(n, 1))
        elif name == "Bernoulli":
            Y.append((rng.rand(n, 1) < 0.5).astype(float))
        elif name == "Poisson":
            Y.append(rng.poisson(3.0, (n, 1)).astype(float))
        elif name in ("Gamma", "Exponential"):
            Y.append(rng.gamma(2.0, 1.0, (n, 1)) + 1e-3)
        elif name == "Beta":
            Y.append(np.clip(rng.beta(2.0, 3.0, (n, 1)), 1e-4, 1 - 1e-4))
        else:
            Y.append(rng.randint(1, kw["K"] + 1, (n, 1)).astype(float))
    h = 1.0 / max(M - 1, 1) if P == 1 else M ** (-1.0 / P)
    if P == 1:
        base = np.linspace(0, 1, M)[:, None]
    else:                      # regular grid (random inducing points make cond(K_uu) ~ 1e6: conditioning-limited parity)
        gsz = int(np.ceil(M ** (1.0 / P)))
        base = np.stack(np.meshgrid(*[np.linspace(0, 1, gsz)] * P, indexing="ij"), -1).reshape(-1, P)[:M]
        h = 1.0 / (gsz - 1)
    Z = np.tile(base, (1, Q)) + 0.1 * h * rng.randn(M, Q * P)
    Lfull = [np.eye(M) * (0.6 + 0.4 * rng.rand(M)) + 0.02 * np.tril(rng.randn(M, M), -1) for _ in range(Q)]
    r, c = np.tril_indices(M)
    prm = dict(Z=Z, m_u=rng.randn(M, Q), L_flat=np.stack([L[r, c] for L in Lfull], 1), variance=0.5 + 0.5 * rng.rand(Q),
               lengthscale=np.array(cs) * h, W=np.where(rng.rand(Q, Df) < 0.5, 1.0, -1.0) * (0.5 + 0.3 * rng.randn(Q, Df)),
               kappa=np.zeros((Q, Df)))
    return prm, prob, X, Y


# ------------------------------------------------------------------------------------------------ the families beyond the reference's
_PROXY = {"Student": ("HetGaussian", {}), "Ordinal": ("Bernoulli", {})}


def family_case(seed, specs, Ns, M, Q, P):
    """(prm, prob, X, Y) of a model with Student / Ordinal / Dirichlet tasks.  `synth` draws a Student task as HetGaussian and an
    Ordinal one as Bernoulli (same dim_f; a Dirichlet task takes its label branch as it is); then, from RandomState(seed + 1) in
    task order, their observations are replaced: Student by heavy-tailed ones with 5 % gross outliers, Ordinal by labels in 1..K,
    Dirichlet by compositions, (N, K)."""
    from oracle import svmogp_oracle as so
    prm, _, X, Y = synth(seed, [_PROXY.get(n, (n, kw)) for n, kw in specs], Ns, M, Q, P, tuple(0.9 + 0.15 * q for q in range(Q)))
    rng = np.random.RandomState(seed + 1)
    for t, (n, kw) in enumerate(specs):
        if n == "Student":
            y = 0.5 * rng.standard_t(kw["deg_free"], (Ns[t], 1))
            out = rng.rand(Ns[t], 1) < 0.05
            Y[t] = np.where(out, y + 20.0 * np.sign(rng.randn(Ns[t], 1)), y)
        elif n == "Ordinal":
            Y[t] = rng.randint(1, kw["K"] + 1, (Ns[t], 1)).astype(float)
        elif n == "Dirichlet":
            y = np.maximum(rng.dirichlet(np.full(kw["K"], 1.5), Ns[t]), 1e-9)
            Y[t] = y / y.sum(1, keepdims=True)
    return prm, so.make_problem(specs, Q, M, P), X, Y


def _parity(out, want, what=""):
    """assert_parity on every array, after printing the worst figures (pytest -s shows them; DESIGN 6 records them)."""
    print("[parity] %-22s worst norm error / 1e-8 = %.3g, worst element-wise excess = %.3g" % (
        what or "full batch", max(rel_norm(out[k], want[k]) for k in KEYS) / 1e-8, max(elementwise_excess(out[k], want[k]) for k in KEYS)))
    for k in KEYS:
        assert_parity(out[k], want[k], what + k)


def _minibatch_oracle(case, Ns, rb, re):
    """(batch scales N / n, the oracle on the row slices [rb, re) of every task)."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = case
    bs = [float(n) / (e - b) for n, b, e in zip(Ns, rb, re)]
    return bs, so.elbo_grad_fused(prm, prob, [x[b:e] for x, b, e in zip(X, rb, re)], [y[b:e] for y, b, e in zip(Y, rb, re)],
                                  batch_scale=bs)


def check_vs_oracle(case, Ns, chunk_rows=97):
    """The default path with one row pool and with several (chunk_rows below the row count), then, on both engines, a minibatch
    whose row_begin > 0 and whose slice is shorter than the task (a per-row array is read with the TASK's stride there)."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = case
    want = so.elbo_grad_fused(prm, prob, X, Y)
    rb = [n // 5 for n in Ns]
    re = [min(n, b + max(1, n // 3)) for n, b in zip(Ns, rb)]
    bs, wantb = _minibatch_oracle(case, Ns, rb, re)
    engines = make_engine(prob, X, Y), make_engine(prob, X, Y, chunk_rows=chunk_rows)
    for e in engines:
        _parity(run(e, prm), want)
    for e in engines:
        _parity(run(e, prm, bs, row_begin=rb, row_end=re), wantb, "minibatch ")
    for e in engines:
        e.close()


def check_small_vs_regular(case, Ns, minibatch):
    """M <= 64: the fused small-model kernels (their hipGraph is the witness: only that path captures one) equal the regular kernels
    (small_path=False) on the same model, both equal the oracle, and so does a minibatch (row_begin, row_end) on the small path,
    replayed from its graph."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = case
    want = so.elbo_grad_fused(prm, prob, X, Y)
    es, er = make_engine(prob, X, Y), make_engine(prob, X, Y, small_path=False)
    for _ in range(3):
        a, b = run(es, prm), run(er, prm)
    assert es.graph_stats()[0] >= 1 and er.graph_stats() == (0, 0), (es.graph_stats(), er.graph_stats())
    worst = {k: rel_norm(a[k], b[k]) for k in KEYS}
    print("small vs regular path, relative difference per array:", {k: "%.1e" % x for k, x in worst.items()})
    assert worst["elbo"] < 1e-12, worst
    for k in KEYS:
        assert worst[k] < 1e-10, (k, worst[k])
    _parity(a, want)
    _parity(b, want, "no small path ")
    rb, re = minibatch
    bs, wantb = _minibatch_oracle(case, Ns, rb, re)
    for _ in range(2):
        outb = run(es, prm, bs, row_begin=rb, row_end=re)
    _parity(outb, wantb, "small-path minibatch ")
    es.close(), er.close()


def check_strict_vs_literal(case):
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = case
    lit = so.elbo_grad_literal(prm, prob, X, Y)
    e = make_engine(prob, X, Y, strict_qf=True)
    out = run(e, prm)
    assert out["rungs"] == [-1, -1]
    _parity(out, lit)
    e.close()
