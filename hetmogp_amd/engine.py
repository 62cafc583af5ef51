"""NumPy-level wrapper of the C ABI (one object = one ``hmogp_handle``): the inner layer of the facade.

Mirrors what ``SVMOGP.parameters_changed`` needs from ``SVMOGPInf.inference`` + the gradient assembly
(reference: hetmogp/svmogp.py:85-166, hetmogp/svmogp_inf.py:23-250): parameters in, ELBO and parameter
gradients out.  All arithmetic happens in ``libhetmogp_hip.so``; this file only marshals arrays.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check

LIK_IDS = dict(Gaussian=_lib.LIK_GAUSSIAN, Bernoulli=_lib.LIK_BERNOULLI, HetGaussian=_lib.LIK_HETGAUSSIAN,
               Categorical=_lib.LIK_CATEGORICAL, Poisson=_lib.LIK_POISSON, Exponential=_lib.LIK_EXPONENTIAL,
               Gamma=_lib.LIK_GAMMA, Beta=_lib.LIK_BETA, Student=_lib.LIK_STUDENT, Ordinal=_lib.LIK_ORDINAL,
               Dirichlet=_lib.LIK_DIRICHLET, NegBinomial=_lib.LIK_NEGBINOMIAL, Weibull=_lib.LIK_WEIBULL,
               Binomial=_lib.LIK_BINOMIAL, BetaBinomial=_lib.LIK_BETABINOMIAL, ZIPoisson=_lib.LIK_ZIPOISSON)

_TWO_COLUMN_Y = {"Weibull": "(time, event indicator)", "Binomial": "(successes k, trials n)", "BetaBinomial": "(successes k, trials n)"}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_lib.c_double_p)


def lik_dim_f(name, **kw):
    """Number of latent parameter functions (the reference's ``get_metadata()[1]``)."""
    if name == "Categorical":
        return int(kw["K"]) - 1
    if name == "Dirichlet":
        return int(kw["K"])
    return dict(Gaussian=1, Bernoulli=1, HetGaussian=2, Poisson=1, Exponential=1, Gamma=2, Beta=2, Student=2, Ordinal=1,
                NegBinomial=2, Weibull=2, Binomial=1, BetaBinomial=2, ZIPoisson=2)[name]


def lik_dim_y(name, **kw):
    """Columns of a task's Y (the reference's ``get_metadata()[0]``): 1, but K for a Dirichlet task and 2 for a Weibull (time, event
    indicator), Binomial or BetaBinomial (successes, trials) task."""
    return int(kw["K"]) if name == "Dirichlet" else (2 if name in _TWO_COLUMN_Y else 1)


def _y_rows(name, y, **kw):
    """y of one task as the library reads it: (N,), or (N, K) row-major for a Dirichlet task, (N, 2) for a Weibull, Binomial or
    BetaBinomial task (whose second column is a flag or a trial count, not an observation: an array of any other shape is refused
    instead of being reshaped into pairs)."""
    dy = lik_dim_y(name, **kw)
    if name in _TWO_COLUMN_Y and (np.ndim(y) != 2 or np.shape(y)[1] != 2):
        raise _lib.InvalidArgument("%s: Y must be (N, 2) = %s, got shape %r" % (name, _TWO_COLUMN_Y[name], np.shape(y)))
    return _f64(y).reshape(-1) if dy == 1 else _f64(y).reshape(-1, dy)


def ordinal_edges(K=None, bin_edges=None):
    """The K - 1 cut points of an Ordinal likelihood: `bin_edges` as given, or the unit-spaced ones centred on 0,
    b_k = k - K/2 (k = 1 .. K-1), when only K is.  Both given must agree.  Their values are checked by the library."""
    if bin_edges is None:
        if K is None:
            raise ValueError("Ordinal needs K or bin_edges")
        return np.arange(1, int(K), dtype=np.float64) - 0.5 * int(K)
    edges = np.array(bin_edges, dtype=np.float64).reshape(-1)
    if K is not None and len(edges) != int(K) - 1:
        raise ValueError("Ordinal: len(bin_edges) = %d does not agree with K = %d" % (len(edges), int(K)))
    return edges


def ordinal_table(K=None, bin_edges=None, sigma=1.0):
    """Registers the cut points and sigma of an Ordinal likelihood with the library (`hmogp_ordinal_table`) and returns the id
    that travels as its `lik_param`.  An identical table gets the same id; an invalid one raises InvalidArgument."""
    edges = ordinal_edges(K, bin_edges)
    out = C.c_double(0.0)
    check(lib.hmogp_ordinal_table(len(edges) + 1, _p(edges), float(sigma), C.byref(out)))
    return float(out.value)


def lik_param(name, **kw):
    if name == "Gaussian":
        s = kw.get("sigma")
        return 0.5 if s is None else float(s)          # gaussian.py:21-24
    if name in ("Categorical", "Dirichlet"):           # (Dirichlet: the library refuses a K outside 2 .. DIRICHLET_MAXK)
        return float(kw["K"])
    if name == "Student":
        return float(kw.get("deg_free", 5.0))          # nu; the library refuses a nu that is not finite and > 0
    if name == "Ordinal":
        if "table_id" in kw:                           # an id from ordinal_table(), passed through as it is
            return float(kw["table_id"])
        return ordinal_table(kw.get("K"), kw.get("bin_edges"), kw.get("sigma", 1.0))
    if name in ("Binomial", "BetaBinomial"):           # the trial count n* of predictive / sample; the library refuses a non-integer
        return float(kw.get("pred_trials", 1))         # or one outside 1 .. 1e9 (0 means 1)
    return 0.0


class _PinnedBlock(object):
    """Owner of one hipHostMalloc allocation; freed when the last NumPy view goes away."""

    def __init__(self, nbytes):
        self.ptr = lib.hmogp_host_alloc(int(nbytes))
        if not self.ptr:
            raise MemoryError("hmogp_host_alloc(%d) failed" % nbytes)
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib.hmogp_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64):
    """NumPy array in page-locked host memory (hmogp_host_alloc): parameters kept in such arrays, and the gradients of an
    ``Engine(reuse_outputs=True)``, move between host and HBM without the driver's staging copy."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if shape else 1
    blk = _PinnedBlock(max(1, n) * dt.itemsize)
    buf = (C.c_char * blk.nbytes).from_address(blk.ptr)
    buf._owner = blk          # every NumPy view keeps `buf` (its base) alive, and with it the allocation
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


class Engine(object):
    """specs: list of (likelihood class name, kwargs) per task, e.g. [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {})]."""

    def __init__(self, specs, Q, M, P, device=0, chunk_rows=0, exact_zero_windows=False, cache_kuu=False, small_path=True,
                 reuse_outputs=False, quirks="reference", strict_qf=False):
        # strict_qf=True (HMOGP_CFG_STRICT_QF): q(f) and the row side of the gradients through the reference's solve-based forms
        # (svmogp_inf.py:214-218, :144-161) instead of the explicit C_q -- parity within 1e-5 also where GPy's jitter ladder is taken
        self.strict_qf = bool(strict_qf)
        self.specs = [(n, dict(k)) for n, k in specs]
        self.T, self.Q, self.M, self.P = len(specs), int(Q), int(M), int(P)
        f_index, d_index = [], []
        for t, (name, kw) in enumerate(self.specs):
            df = lik_dim_f(name, **kw)
            f_index += [t] * df
            d_index += list(range(df))
        self.f_index = np.array(f_index, dtype=np.int32)
        self.d_index = np.array(d_index, dtype=np.int32)
        self.Df = len(f_index)
        self.Mtri = self.M * (self.M + 1) // 2
        lik_id = np.array([LIK_IDS[n] for n, _ in self.specs], dtype=np.int32)
        lik_par = np.array([lik_param(n, **k) for n, k in self.specs], dtype=np.float64)
        cfg = _lib.Config(_lib.ABI_VERSION, self.T, self.Q, self.M, self.P, self.Df,
                          lik_id.ctypes.data_as(_lib.c_int32_p), _p(lik_par),
                          self.f_index.ctypes.data_as(_lib.c_int32_p), self.d_index.ctypes.data_as(_lib.c_int32_p),
                          int(device), int(chunk_rows),
                          (_lib.CFG_EXACT_ZERO_WINDOWS if exact_zero_windows else 0) | (_lib.CFG_CACHE_KUU if cache_kuu else 0) |
                          (0 if small_path else _lib.CFG_NO_SMALL_PATH) | (_lib.CFG_STRICT_QF if strict_qf else 0),
                          _lib.quirk_mask(quirks))
        self.quirks = _lib.quirk_mask(quirks)
        self._h = C.c_void_p()
        check(lib.hmogp_create(C.byref(cfg), C.byref(self._h)), None)
        self.N = [0] * self.T
        self.last = None
        # reuse_outputs=True: g_m_u / g_L_u / g_Z are returned as views of page-locked arrays owned by the engine (DMA
        # without the driver's staging copy), and the small outputs as engine-owned arrays too (the hmogp_outputs struct is
        # built once: ~25 us of ctypes work per call otherwise); ALL are overwritten by the next evaluation -- copy what
        # must persist.
        self.reuse_outputs = bool(reuse_outputs)
        self._pcache = None
        self._ocache = {}
        self._pinned_out = None
        self._paths_shape = {}           # live path sets: slot id -> (size, nD, num_features)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib.hmogp_destroy(self._h)
            self._h = None
            self._paths_shape = {}      # (the engine's path sets went with it)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------ data
    def set_task_data(self, t, X, Y):
        X, Y = _f64(X).reshape(-1, self.P), _y_rows(self.specs[t][0], Y, **self.specs[t][1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y of task %d have different lengths" % t)
        check(lib.hmogp_set_task_data(self._h, t, _p(X), _p(Y), X.shape[0]), self._h)
        self.N[t] = X.shape[0]

    def set_data(self, X_list, Y_list):
        for t, (X, Y) in enumerate(zip(X_list, Y_list)):
            self.set_task_data(t, X, Y)

    # ------------------------------------------------------------------------------------------ params
    def _params(self, Z, m_u, L_flat, variance, lengthscale, W, kappa, W0=None, kappa0=None, batch_scale=None,
                row_begin=None, row_end=None, forced_rung=None, group_mask=_lib.GROUP_ALL, strict_qf=None, skip_g_L=False):
        """hmogp_params for one call.  The struct and the addresses of the arrays it points to are kept between calls: an
        argument that is THE SAME C-contiguous array object as last time (an optimiser updating its parameters in place) costs
        one identity check; anything else is converted (copied if it has to be) and its address taken again."""
        Q, M, P, Df, T = self.Q, self.M, self.P, self.Df, self.T
        if self._pcache is None:
            f8, i8, i4 = np.dtype(np.float64), np.dtype(np.int64), np.dtype(np.int32)
            spec = dict(Z=(M * Q * P, f8), m_u=(M * Q, f8), L_flat=(self.Mtri * Q, f8), variance=(Q, f8), lengthscale=(Q, f8),
                        W=(Q * Df, f8), kappa=(Q * Df, f8), W0=(Q * Df, f8), kappa0=(Q * Df, f8), batch_scale=(T, f8),
                        row_begin=(T, i8), row_end=(T, i8), forced_rung=(Q, i4))
            self._pcache = (_lib.Params(), spec, {k: None for k in spec}, {})
        p, spec, last, keep = self._pcache
        for k, a in (("Z", Z), ("m_u", m_u), ("L_flat", L_flat), ("variance", variance), ("lengthscale", lengthscale), ("W", W),
                     ("kappa", kappa), ("W0", W0), ("kappa0", kappa0), ("batch_scale", batch_scale), ("row_begin", row_begin),
                     ("row_end", row_end), ("forced_rung", forced_rung)):
            if a is last[k] and a is not None:
                continue
            if a is None:
                setattr(p, k, None)
                last[k] = keep[k] = None
                continue
            size, dt = spec[k]
            b = a if (type(a) is np.ndarray and a.dtype == dt and a.flags.c_contiguous) else np.ascontiguousarray(a, dtype=dt)
            if b.size != size:
                raise ValueError("%s: expected %d elements, got an array of shape %s" % (k, size, np.shape(a)))
            setattr(p, k, b.ctypes.data)
            keep[k] = b
            last[k] = a if b is a else None      # (a converted copy does not follow later in-place changes of `a`: convert again)
        p.group_mask = int(group_mask)
        p.eval_flags = (_lib.EVAL_STRICT_QF if strict_qf else 0) | (_lib.EVAL_NO_G_L if skip_g_L else 0)   # (per evaluation)
        return p, keep

    def _outputs(self, want_dL_dS=False, skip_qu=False):
        Q, M, P, Df = self.Q, self.M, self.P, self.Df
        key = (bool(want_dL_dS), bool(skip_qu))
        if self.reuse_outputs and key in self._ocache:     # every output array is owned by the engine and overwritten by the
            c, o = self._ocache[key]                        # next evaluation; the struct pointing at them is built once
            return c, dict(o)
        if self.reuse_outputs:      # page-locked arrays owned by the engine, overwritten by the next evaluation
            if self._pinned_out is None:
                self._pinned_out = dict(g_m_u=pinned_empty((M, Q)), g_L_u=pinned_empty((self.Mtri, Q)),
                                        g_Z=pinned_empty((M, Q * P)))
            big = self._pinned_out
        else:
            big = dict(g_m_u=np.zeros((M, Q)), g_L_u=np.zeros((self.Mtri, Q)), g_Z=np.zeros((M, Q * P)))
        o = dict(elbo=np.zeros(1), g_m_u=big["g_m_u"], g_L_u=big["g_L_u"], g_variance=np.zeros(Q),
                 g_lengthscale=np.zeros(Q), g_W=np.zeros((Q, Df)), g_kappa=np.zeros((Q, Df)), g_Z=big["g_Z"], kl=np.zeros(Q),
                 cond_est=np.zeros(Q))
        if want_dL_dS:
            o["dL_dS"] = np.zeros((Q, M, M))
        rung = np.zeros(Q, dtype=np.int32)
        flags = np.zeros(1, dtype=np.uint32)
        c = _lib.Outputs()
        for k, v in o.items():
            setattr(c, k, v.ctypes.data)
        if not want_dL_dS:
            c.dL_dS = None
        if skip_qu:                  # q(u) is device-resident: its gradient stays in HBM for hmogp_qu_adadelta
            c.g_m_u = None
            c.g_L_u = None
            o["g_m_u"] = o["g_L_u"] = None
        c.rung = rung.ctypes.data
        c.flags = flags.ctypes.data
        o["rung"], o["flags"] = rung, flags
        if self.reuse_outputs:
            self._ocache[key] = (c, dict(o))
        return c, o

    def _wrap(self, o):
        res = dict(o)
        res["elbo"] = float(o["elbo"][0])
        res["KL"] = float(np.sum(o["kl"]))          # calculate_KL (svmogp_inf.py:227-250), summed over the latents
        res["rungs"] = [int(r) for r in o["rung"]]
        res["v_negative"] = bool(int(o["flags"][0]) & _lib.FLAG_V_NEGATIVE)
        # cond_est[q] = variance_q max_i (K_uu^-1)_ii (lower bound of cond(K_uu), 30-150x below it); ill_conditioned: beyond what this
        # engine's mode keeps within element-wise 1e-5 of the reference (default mode: take strict_qf=True)
        res["ill_conditioned"] = bool(int(o["flags"][0]) & _lib.FLAG_ILL_CONDITIONED)
        self.last = res
        return res

    # ------------------------------------------------------------------------------------------ hot path
    def elbo_grad(self, want_dL_dS=False, sharded=False, **params):
        """One ``parameters_changed()``: returns dict(elbo, KL, kl [Q], g_m_u, g_L_u, g_variance, g_lengthscale, g_W,
        g_kappa, g_Z, rungs, v_negative[, dL_dS]).  `sharded=True` = hmogp_elbo_grad_sharded: the row-sharded step of a
        multi-GPU run (begin on this rank's rows -> in-library all-reduce -> finish), COLLECTIVE over the ranks of the
        communicator attached with `comm_init`; the default never communicates.
        With `Engine(reuse_outputs=True)` EVERY returned array (the three large gradients AND the small ones: g_variance, g_W,
        kl, rung, flags ...) is owned by the engine and overwritten in place by the next evaluation -- `engine.last` and any
        retained result dict change with it; copy what must persist."""
        p, keep = self._params(**params)
        c, o = self._outputs(want_dL_dS, skip_qu=params.get("m_u") is None)
        fn = lib.hmogp_elbo_grad_sharded if sharded else lib.hmogp_elbo_grad
        check(fn(self._h, C.byref(p), C.byref(c)), self._h)
        return self._wrap(o)

    def step_begin(self, **params):
        self._skip_qu = params.get("m_u") is None      # device-resident q(u): step_finish leaves its gradient in HBM too
        p, keep = self._params(**params)
        check(lib.hmogp_step_begin(self._h, C.byref(p)), self._h)

    def stats_buffer(self):
        """(device pointer, float64 count) of the additive statistic bundle -- what a multi-GPU run all-reduces."""
        ptr, n = C.c_void_p(), C.c_int64()
        check(lib.hmogp_stats_buffer(self._h, C.byref(ptr), C.byref(n)), self._h)
        return ptr.value, n.value

    def stats_read(self):
        _, n = self.stats_buffer()
        out = np.zeros(n)
        check(lib.hmogp_stats_read(self._h, _p(out)), self._h)
        return out

    def stats_write(self, host):
        host = _f64(host)
        check(lib.hmogp_stats_write(self._h, _p(host)), self._h)

    def wire_buffer(self):
        """(device pointer, float64 count) of the wire format of the bundle (lower triangles of H_q only)."""
        ptr, n = C.c_void_p(), C.c_int64()
        check(lib.hmogp_wire_buffer(self._h, C.byref(ptr), C.byref(n)), self._h)
        return ptr.value, n.value

    def wire_pack(self):
        check(lib.hmogp_wire_pack(self._h), self._h)

    def wire_unpack(self):
        check(lib.hmogp_wire_unpack(self._h), self._h)

    def wire_read(self):
        _, n = self.wire_buffer()
        out = np.zeros(n)
        check(lib.hmogp_wire_read(self._h, _p(out)), self._h)
        return out

    def wire_write(self, host):
        host = _f64(host)
        check(lib.hmogp_wire_write(self._h, _p(host)), self._h)

    # ------------------------------------------------------------------------------------------ native exchange
    def comm_init(self, nranks, rank, unique_id):
        """Attach an RCCL communicator (collective: every rank, same `unique_id` from `comm_unique_id()` of ONE rank).
        From then on `elbo_grad(sharded=True)` is the row-sharded step: begin -> in-library all-reduce -> finish."""
        uid = bytes(unique_id)
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % _lib.COMM_ID_BYTES)
        buf = C.create_string_buffer(uid, _lib.COMM_ID_BYTES)
        check(lib.hmogp_comm_init(self._h, int(nranks), int(rank), buf), self._h)

    def comm_destroy(self):
        check(lib.hmogp_comm_destroy(self._h), self._h)

    def comm_info(self):
        n, r = C.c_int32(), C.c_int32()
        check(lib.hmogp_comm_info(self._h, C.byref(n), C.byref(r)), self._h)
        return n.value, r.value

    def step_exchange(self):
        """Enqueue pack -> RCCL all-reduce -> unpack on the engine's stream (between step_begin and step_finish)."""
        check(lib.hmogp_step_exchange(self._h), self._h)

    def step_finish(self, want_dL_dS=False):
        c, o = self._outputs(want_dL_dS, skip_qu=getattr(self, "_skip_qu", False))
        check(lib.hmogp_step_finish(self._h, C.byref(c)), self._h)
        return self._wrap(o)

    # ------------------------------------------------------------------------------------------ consumers
    def posterior_u(self):
        wv = np.zeros((self.Q, self.M))
        wi = np.zeros((self.Q, self.M, self.M))
        check(lib.hmogp_posterior_u(self._h, _p(wv), _p(wi)), self._h)
        return wv, wi

    def natgrad_step(self, gamma=1.0):
        """Natural-gradient update of q(u) from the last evaluation's gradients: returns (m_u_new, L_flat_new)."""
        m = np.zeros((self.M, self.Q))
        L = np.zeros((self.Mtri, self.Q))
        check(lib.hmogp_natgrad_step(self._h, float(gamma), _p(m), _p(L)), self._h)
        return m, L

    def predict_f(self, Xnew):
        Xnew = _f64(Xnew).reshape(-1, self.P)
        m = np.zeros((Xnew.shape[0], self.Df))
        v = np.zeros((Xnew.shape[0], self.Df))
        check(lib.hmogp_predict_f(self._h, _p(Xnew), Xnew.shape[0], _p(m), _p(v)), self._h)
        return m, v

    def _joint_functions(self, functions):
        d = np.arange(self.Df) if functions is None else np.asarray(functions).reshape(-1)
        if d.size and not np.issubdtype(d.dtype, np.integer):
            raise _lib.InvalidArgument("functions must be integer indices")
        return np.ascontiguousarray(d, dtype=np.int32)

    def predict_f_joint(self, Xnew, functions=None):
        """The joint posterior of the functions `functions` (None: all Df) at Xnew: (mean (nD, N), cov (nD, N, nD, N)),
        cov exactly symmetric as an (nD N) x (nD N) matrix; nD * N <= _lib.JOINT_MAXDIM."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        d = self._joint_functions(functions)
        N, nD = Xnew.shape[0], d.shape[0]
        mean = np.zeros((nD, N))
        cov = np.zeros((nD * N, nD * N)) if nD * N <= _lib.JOINT_MAXDIM else np.zeros((0, 0))     # (beyond the limit the call is refused)
        check(lib.hmogp_predict_f_joint(self._h, _p(Xnew), N, nD, d.ctypes.data_as(_lib.c_int32_p), _p(mean), _p(cov)), self._h)
        return mean, cov.reshape(nD, N, nD, N)

    def sample_f_joint(self, Xnew, functions=None, size=1, seed=0, return_factor=False):
        """`size` joint draws F[s] = mean + L z_s of the same Gaussian: (size, nD, N).  L = chol(cov + jitter I) on the ladder of
        `jitchol_inv`; z_s[i] is the counter-based normal at (seed, row i, sample s), so draw s does not depend on `size`.
        return_factor=True: (F, dict(mean (nD, N), L (nD N, nD N), jitter, rung)) -- rung -1 / jitter 0: the plain factorisation."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        d = self._joint_functions(functions)
        N, nD, S = Xnew.shape[0], d.shape[0], int(size)
        n = nD * N
        ok = n <= _lib.JOINT_MAXDIM and S >= 1
        F = np.zeros((S, nD, N)) if ok else np.zeros((1, 0, 0))
        mean = np.zeros((nD, N))
        L = np.zeros((n, n)) if (return_factor and ok) else None
        jit, rung = C.c_double(0.0), C.c_int32(-1)
        check(lib.hmogp_sample_f_joint(self._h, _p(Xnew), N, nD, d.ctypes.data_as(_lib.c_int32_p), S, int(seed) & (2 ** 64 - 1), _p(F),
                                       _p(mean), _p(L) if L is not None else None, C.byref(jit), C.byref(rung)), self._h)
        if return_factor:
            return F, dict(mean=mean, L=L, jitter=float(jit.value), rung=int(rung.value))
        return F

    # pathwise (Matheron) posterior samples: a path set is drawn once and evaluated anywhere, any number of times
    def paths_create(self, functions=None, size=1, num_features=1024, seed=0):
        """Draw a path set -- `size` sample paths of the functions `functions` (None: all Df) with `num_features` random Fourier
        frequencies per latent -- from the parameters of the last evaluation; returns its id.  At most _lib.PATHS_MAXSETS live sets."""
        d = self._joint_functions(functions)
        sid = C.c_int32(-1)
        check(lib.hmogp_paths_create(self._h, d.shape[0], d.ctypes.data_as(_lib.c_int32_p), int(size), int(num_features),
                                     int(seed) & (2 ** 64 - 1), C.byref(sid)), self._h)
        self._paths_shape[int(sid.value)] = (int(size), d.shape[0], int(num_features))
        return int(sid.value)

    def _paths_dims(self, sid):
        dims = self._paths_shape.get(int(sid))
        if dims is None:       # (the library refuses the id with its own message)
            check(lib.hmogp_paths_eval(self._h, int(sid), None, 0, None), self._h)
            raise _lib.InvalidArgument("paths: unknown or freed path-set id")
        return dims

    def paths_eval(self, sid, Xnew):
        """The paths of set `sid` at Xnew: (size, nD, N), the layout of `sample_f_joint`; the same function on every call, any N."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        S, nD, _ = self._paths_dims(sid)
        F = np.zeros((S, nD, Xnew.shape[0]))
        check(lib.hmogp_paths_eval(self._h, int(sid), _p(Xnew), Xnew.shape[0], _p(F)), self._h)
        return F

    def paths_eval_grad(self, sid, Xnew, values=False):
        """The gradients of the paths of set `sid` with respect to the inputs: G (size, nD, N, P), G[s, j, i, p] = d f / d x_p at
        row i; with values=True (F, G), F the bits of `paths_eval`."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        S, nD, _ = self._paths_dims(sid)
        G = np.zeros((S, nD, Xnew.shape[0], self.P))
        F = np.zeros((S, nD, Xnew.shape[0])) if values else None
        check(lib.hmogp_paths_eval_grad(self._h, int(sid), _p(Xnew), Xnew.shape[0], _p(F) if values else None, _p(G)), self._h)
        return (F, G) if values else G

    def paths_state(self, sid):
        """The set's state: dict(omega (Q, Lf, P), theta (Q, 2 Lf, S, nD) = W theta + sqrt(kappa) theta', v (Q, M, S, nD) = W v, u (Q, S, M))."""
        S, nD, Lf = self._paths_dims(sid)
        out = dict(omega=np.zeros((self.Q, Lf, self.P)), theta=np.zeros((self.Q, 2 * Lf, S, nD)), v=np.zeros((self.Q, self.M, S, nD)),
                   u=np.zeros((self.Q, S, self.M)))
        check(lib.hmogp_paths_state(self._h, int(sid), _p(out["omega"]), _p(out["theta"]), _p(out["v"]), _p(out["u"])), self._h)
        return out

    def paths_free(self, sid):
        check(lib.hmogp_paths_free(self._h, int(sid)), self._h)
        self._paths_shape.pop(int(sid), None)

    def predict_f_grad(self, Xnew, return_mv=False):
        """Gradients of q(f) with respect to the inputs Xnew: (dm (N, Df, P), dv (N, Df, P)), dm[i, d, j] = d m_d / d x_j and
        dv[i, d, j] = d v_d / d x_j at row i, in the mode of the evaluation they are taken from.  v is the SIGNED variance `predict_f`
        returns (before any abs).  return_mv=True: (m, v, dm, dv) with m, v the bits of `predict_f`."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        N = Xnew.shape[0]
        dm, dv = np.zeros((N, self.Df, self.P)), np.zeros((N, self.Df, self.P))
        m = np.zeros((N, self.Df)) if return_mv else None
        v = np.zeros((N, self.Df)) if return_mv else None
        check(lib.hmogp_predict_f_grad(self._h, _p(Xnew), N, _p(m) if return_mv else None, _p(v) if return_mv else None, _p(dm), _p(dv)),
              self._h)
        return (m, v, dm, dv) if return_mv else (dm, dv)

    # ------------------------------------------------------------------------------------------ resident q(u)
    def qu_load(self, m_u, L_flat):
        m_u, L_flat = _f64(m_u).reshape(self.M, self.Q), _f64(L_flat).reshape(self.Mtri, self.Q)
        check(lib.hmogp_qu_load(self._h, _p(m_u), _p(L_flat)), self._h)

    def qu_read(self):
        m, L = np.zeros((self.M, self.Q)), np.zeros((self.Mtri, self.Q))
        check(lib.hmogp_qu_read(self._h, _p(m), _p(L)), self._h)
        return m, L

    def qu_natgrad(self, gamma=1.0):
        """Natural-gradient step on the DEVICE-RESIDENT q(u) (hmogp_qu_natgrad): in place in HBM, from the gradients of the
        last evaluation.  Raises LinAlgError (HMOGP_E_NOT_PD) with q(u) untouched when gamma is too large."""
        check(lib.hmogp_qu_natgrad(self._h, float(gamma)), self._h)

    def qu_natgrad_async(self, gamma=1.0):
        """hmogp_qu_natgrad_async (ABI v7): the same step without the host synchronisation -- committed on the device only if it
        stays inside the positive-definite cone; `qu_natgrad_status()` tells later.  The next evaluation may be enqueued at once."""
        check(lib.hmogp_qu_natgrad_async(self._h, float(gamma)), self._h)

    def qu_natgrad_status(self):
        """True if the last asynchronous natural-gradient step was committed (waits for it if it is still pending)."""
        t = C.c_int32(0)
        check(lib.hmogp_qu_natgrad_status(self._h, C.byref(t)), self._h)
        return bool(t.value)

    def qu_adadelta(self, phase, step_rate, momentum, decay, offset):
        check(lib.hmogp_qu_adadelta(self._h, int(phase), float(step_rate), float(momentum), float(decay), float(1 - decay),
                                    float(offset)), self._h)

    def debug_raw_grads(self, rows):
        """The reference's inner-protocol gradient dict of the last evaluation (small N, one pool, GROUP_ALL):
        rows[t] = rows of task t in that evaluation.  Returns dict(dL_dKmm [Q][M,M], dL_dKmn [Q][Df][M,N_t],
        dL_dKdiag [Q][Df][N_t])."""
        Q, M, Df = self.Q, self.M, self.Df
        nd = [int(rows[self.f_index[d]]) for d in range(Df)]
        kmm = np.zeros((Q, M, M))
        kmn = np.zeros(Q * M * sum(nd))
        kdg = np.zeros(Q * sum(nd))
        check(lib.hmogp_debug_raw_grads(self._h, _p(kmm), _p(kmn), _p(kdg)), self._h)
        out = dict(dL_dKmm=[kmm[q] for q in range(Q)], dL_dKmn=[], dL_dKdiag=[])
        o1 = o2 = 0
        for q in range(Q):
            a, b = [], []
            for d in range(Df):
                a.append(kmn[o1:o1 + M * nd[d]].reshape(M, nd[d]))
                b.append(kdg[o2:o2 + nd[d]].copy())
                o1 += M * nd[d]
                o2 += nd[d]
            out["dL_dKmn"].append(a)
            out["dL_dKdiag"].append(b)
        return out

    # ------------------------------------------------------------------------------------------ likelihood parameters
    def lik_param_count(self, t):
        """Parameters task t's likelihood can learn: 1 (Gaussian sigma, Student deg_free), K (Ordinal: K - 1 cuts, then sigma), else 0."""
        cache = self.__dict__.setdefault("_lik_counts", {})      # (fixed at construction: K does not change)
        if t not in cache:
            n = C.c_int32(0)
            check(lib.hmogp_lik_param_count(self._h, int(t), C.byref(n)), self._h)
            cache[t] = int(n.value)
        return cache[t]

    def set_lik_params(self, t, values):
        """New values of task t's likelihood parameters (layout of `lik_param_count`); InvalidArgument leaves the task unchanged."""
        values = _f64(values).reshape(-1)
        check(lib.hmogp_set_lik_params(self._h, int(t), _p(values), values.shape[0]), self._h)

    def lik_grad_enable(self, on=True):
        """Persistent switch: evaluations whose group_mask holds GROUP_HYPER also compute d ELBO / d (likelihood parameters)."""
        check(lib.hmogp_lik_grad_enable(self._h, 1 if on else 0), self._h)

    def lik_grad(self, t):
        """d ELBO / d theta of task t from the last evaluation (zeros when gated or switched off)."""
        g = np.zeros(self.lik_param_count(t))
        check(lib.hmogp_lik_grad_read(self._h, int(t), _p(g), g.shape[0]), self._h)
        return g

    def predict_log_density(self, t, Xnew, Ynew, gh_T=0):
        """(lpd, ess) of task t's new rows (hmogp_predict_log_density): q(f) at Xnew stays on the device and feeds the
        deterministic rule with the task's CURRENT likelihood parameters.  Ynew as set_data takes it for that task."""
        name, kw = self.specs[int(t)] if 0 <= int(t) < self.T else ("Gaussian", {})
        Xnew = _f64(Xnew).reshape(-1, self.P)
        Ynew = _y_rows(name, Ynew, **kw)
        n = Xnew.shape[0]
        if Ynew.shape[0] != n:
            raise _lib.InvalidArgument("predict_log_density: Xnew has %d rows, Ynew %d" % (n, Ynew.shape[0]))
        lpd, ess = np.zeros(n), np.zeros(n)
        check(lib.hmogp_predict_log_density(self._h, int(t), _p(Xnew), _p(Ynew), n, int(gh_T), _p(lpd), _p(ess)), self._h)
        return lpd, ess

    def predict_cdf(self, t, Xnew, ynew, gh_T=0):
        """(cdf, sf) of task t's new rows (hmogp_predict_cdf): q(f) at Xnew stays on the device and feeds the cdf kernels with
        the task's CURRENT likelihood parameters.  ynew: (N,) values (Ordinal: labels; Weibull: times, no indicator column)."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        ynew = _f64(ynew).reshape(-1)
        n = Xnew.shape[0]
        if ynew.shape[0] != n:
            raise _lib.InvalidArgument("predict_cdf: Xnew has %d rows, ynew %d" % (n, ynew.shape[0]))
        cdf, sf = np.zeros(n), np.zeros(n)
        check(lib.hmogp_predict_cdf(self._h, int(t), _p(Xnew), _p(ynew), n, int(gh_T), _p(cdf), _p(sf)), self._h)
        return cdf, sf

    def predict_quantile(self, t, Xnew, probs, gh_T=0):
        """(N, len(probs)) quantiles of task t's new rows (hmogp_predict_quantile); probs in (0, 1), any number of them
        (the library takes _lib.QUANT_MAXP per call)."""
        Xnew = _f64(Xnew).reshape(-1, self.P)
        probs = _f64(probs).reshape(-1)
        n = Xnew.shape[0]
        out = np.zeros((n, probs.shape[0]))
        for c0 in range(0, max(probs.shape[0], 1), _lib.QUANT_MAXP):
            pc = np.ascontiguousarray(probs[c0:c0 + _lib.QUANT_MAXP])
            qc = np.zeros((n, pc.shape[0]))
            check(lib.hmogp_predict_quantile(self._h, int(t), _p(Xnew), n, pc.shape[0], _p(pc), int(gh_T), _p(qc)), self._h)
            out[:, c0:c0 + pc.shape[0]] = qc
        return out

    def graph_stats(self):
        """(graphs captured, evaluations replayed) of the small-model hipGraph mechanism (hmogp_graph_stats)."""
        cap, rep = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        check(lib.hmogp_graph_stats(self._h, cap.ctypes.data_as(_lib.c_int64_p), rep.ctypes.data_as(_lib.c_int64_p)), self._h)
        return int(cap[0]), int(rep[0])

    def timings(self):
        ms = np.zeros(_lib.NTIMINGS)
        n = np.zeros(_lib.NTIMINGS, dtype=np.int64)
        check(lib.hmogp_last_timings(self._h, _p(ms), n.ctypes.data_as(_lib.c_int64_p)), self._h)
        names = ["total", "rbf_cross_cov", "forward_gemm", "rowstats_combine", "quadrature", "gram_gemm", "colstats_reduce",
                 "mxm_algebra", "exchange", "trsm_solves", "strict_rowstats"]   # (the last two: strict q(f) mode only, ABI v8)
        return dict(zip(names, ms.tolist())), dict(zip(names, n.tolist()))


_DEFAULT_DEVICE = 0


_DEFAULT_DEVICE_PINNED = False


def set_default_device(device, from_model=False):
    """HIP device of the stand-alone building blocks below (var_exp, predictive, sample, gemm ...) when they are called
    without `device=`: a rank of a multi-GPU run sets it to its LOCAL_RANK once (SVMOGP(distributed=True) does), so that
    likelihood-level helpers never land on GPU 0 from every rank.  A model constructor (`from_model=True`) only sets
    it while nobody has chosen one explicitly and no earlier model has: with two models on two devices in one process the
    stand-alone helpers of the first no longer move to the GPU of the last; a model's OWN calls always pass its device."""
    global _DEFAULT_DEVICE, _DEFAULT_DEVICE_PINNED
    if from_model and _DEFAULT_DEVICE_PINNED:
        return
    _DEFAULT_DEVICE = int(device)
    _DEFAULT_DEVICE_PINNED = True


def _resolve_device(device):
    return _DEFAULT_DEVICE if device is None else int(device)


def comm_available():
    """True if the library can load librccl (needed only for multi-GPU runs)."""
    return bool(lib.hmogp_comm_available())


def comm_unique_id():
    """ncclGetUniqueId through the library: call on ONE rank, broadcast the bytes, pass them to Engine.comm_init."""
    buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
    check(lib.hmogp_comm_unique_id(buf))
    return buf.raw


# ---------------------------------------------------------------------------------------------- building blocks
def rbf_cross_cov(X, Z, variance, lengthscale, device=None, exact=True):
    """K = k(X, Z).  exact=True: GPy's rounding order (the K_uu variant); exact=False: the hot-path K_uf variant."""
    device = _resolve_device(device)
    X, Z = _f64(X), _f64(Z)
    X = X.reshape(X.shape[0], -1)
    Z = Z.reshape(Z.shape[0], -1)
    K = np.zeros((X.shape[0], Z.shape[0]))
    check(lib.hmogp_rbf_cross_cov_ex(device, _p(X), X.shape[0], _p(Z), Z.shape[0], X.shape[1], float(variance),
                                     float(lengthscale), 1 if exact else 0, _p(K)))
    return K


def kuf_windows_rows(X, Z, lengthscale, device=None):
    """The exact-zero windows of k(X, Z) as the engine's windows mode computes them for one row range and one latent
    (hmogp_kuf_windows): (rowwin [ceil(N / 128), 2], colwin [ceil(M / 128), 2]), int32."""
    device = _resolve_device(device)
    X, Z = _f64(X), _f64(Z)
    X = X if X.ndim == 2 else X.reshape(X.shape[0], -1)
    Z = Z if Z.ndim == 2 else Z.reshape(Z.shape[0], -1)
    N, M, P = X.shape[0], Z.shape[0], X.shape[1]
    rowwin = np.zeros(((N + 127) // 128, 2), dtype=np.int32)
    colwin = np.zeros(((M + 127) // 128, 2), dtype=np.int32)
    check(lib.hmogp_kuf_windows(device, _p(X), N, P, _p(Z), Z.shape[1], M, float(lengthscale), rowwin.ctypes.data_as(_lib.c_int32_p),
                                colwin.ctypes.data_as(_lib.c_int32_p)))
    return rowwin, colwin


def jitchol_inv(A, forced_rung=None, device=None):
    device = _resolve_device(device)
    A = _f64(A)
    Q, M = A.shape[0], A.shape[1]
    L, Ai = np.zeros_like(A), np.zeros_like(A)
    rung = np.zeros(Q, dtype=np.int32)
    fr = None if forced_rung is None else np.ascontiguousarray(forced_rung, dtype=np.int32)
    check(lib.hmogp_jitchol_inv(device, _p(A), Q, M, fr.ctypes.data_as(_lib.c_int32_p) if fr is not None else None,
                                _p(L), _p(Ai), rung.ctypes.data_as(_lib.c_int32_p)))
    return L, Ai, [int(r) for r in rung]


def potri(L, device=None):
    device = _resolve_device(device)
    L = _f64(L)
    out = np.zeros_like(L)
    check(lib.hmogp_potri(device, _p(L), L.shape[0], L.shape[1], _p(out)))
    return out


def potrs_rows(L, B, device=None):
    """B (L L^T)^-1 for the rows of B [n, M]: GPy's dpotrs(L, B^T)^T (svmogp_inf.py:214) by blocked substitution on the device."""
    device = _resolve_device(device)
    L, B = _f64(L), _f64(B)
    out = np.zeros_like(B)
    check(lib.hmogp_potrs_rows(device, _p(L), L.shape[0], _p(B), B.shape[0], _p(out)))
    return out


def gemm(A, B, transA=False, transB=False, alpha=1.0, beta=0.0, C0=None, device=None):
    device = _resolve_device(device)
    A, B = _f64(A), _f64(B)
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    N = B.shape[0] if transB else B.shape[1]
    Cm = np.zeros((M, N)) if C0 is None else _f64(C0).copy()
    check(lib.hmogp_gemm_f64(device, int(transA), int(transB), M, N, K, float(alpha), _p(A), A.shape[1], _p(B), B.shape[1],
                             float(beta), _p(Cm), N))
    return Cm


def var_exp(name, y, m, v, device=None, quirks="reference", **kw):
    device = _resolve_device(device)
    y, m, v = _y_rows(name, y, **kw), _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    ve, dm, dv = np.zeros(y.shape[0]), np.zeros_like(m), np.zeros_like(v)
    check(lib.hmogp_var_exp_ex(device, LIK_IDS[name], lik_param(name, **kw), _lib.quirk_mask(quirks), y.shape[0], _p(y),
                               _p(m), _p(v), _p(ve), _p(dm), _p(dv)))
    return ve, dm, dv


def var_exp_dparam(name, y, m, v, device=None, **kw):
    """Per-row derivatives of the variational expectation with respect to the likelihood's own parameters: (N, 1) for Gaussian
    (d sigma) and Student (d deg_free), (N, 3) for Ordinal (d lo, d hi, d sigma of the row's own two cut points)."""
    device = _resolve_device(device)
    y, m, v = _y_rows(name, y, **kw), _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    cols = dict(Gaussian=1, Student=1, Ordinal=3).get(name, 1)
    out = np.zeros((y.shape[0], cols))
    check(lib.hmogp_var_exp_dparam(device, LIK_IDS[name], lik_param(name, **kw), y.shape[0], _p(y), _p(m), _p(v), _p(out)))
    return out


def predictive(name, m, v, gh_T=0, device=None, **kw):
    """`<likelihood>.predictive(m, v)`: predictive mean / variance of y (N, dim_p)."""
    device = _resolve_device(device)
    m, v = _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    Jp = J if name in ("Categorical", "Dirichlet") else 1
    mean, var = np.zeros((m.shape[0], Jp)), np.zeros((m.shape[0], Jp))
    check(lib.hmogp_predictive(device, LIK_IDS[name], lik_param(name, **kw), int(gh_T), m.shape[0], _p(m), _p(v), _p(mean),
                               _p(var)))
    return mean, var


def log_predictive_rows(name, y, m, v, num_samples=1000, seed=0, device=None, **kw):
    """Per-row Monte-Carlo log predictive density: -log S + logsumexp_s log p(y_n | f_s), f_s ~ N(m_n, diag v_n)."""
    device = _resolve_device(device)
    y, m, v = _y_rows(name, y, **kw), _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    out = np.zeros(y.shape[0])
    check(lib.hmogp_log_predictive(device, LIK_IDS[name], lik_param(name, **kw), y.shape[0], int(num_samples), int(seed),
                                   _p(y), _p(m), _p(v), _p(out)))
    return out


def log_predictive_density_rows(name, y, m, v, gh_T=0, return_ess=False, device=None, **kw):
    """Deterministic per-row log predictive density: the log of the Gauss-Hermite tensor rule of p(y_n | f) under
    q(f) = N(m_n, diag v_n), gh_T nodes per dimension (0: 20, Categorical / Dirichlet 10).  Every family, Gamma and Beta included.
    return_ess=True: (lpd, ess), ess = the rule's effective number of nodes per row (next to 1: the rule cannot resolve the row)."""
    device = _resolve_device(device)
    y, m, v = _y_rows(name, y, **kw), _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    lpd = np.zeros(y.shape[0])
    ess = np.zeros(y.shape[0]) if return_ess else None
    check(lib.hmogp_log_predictive_gh(device, LIK_IDS[name], lik_param(name, **kw), int(gh_T), y.shape[0], _p(y), _p(m), _p(v),
                                      _p(lpd), _p(ess) if return_ess else None))
    return (lpd, ess) if return_ess else lpd


PREDQ_FAMILIES = ("Gaussian", "HetGaussian", "Bernoulli", "Exponential", "Ordinal", "Weibull")
PREDQ_MISSING = {"Poisson": "a regularised incomplete gamma function", "Gamma": "a regularised incomplete gamma function",
                 "Beta": "a regularised incomplete beta function", "Student": "a regularised incomplete beta function",
                 "NegBinomial": "a regularised incomplete beta function", "Categorical": "an order of its classes (it has none)",
                 "Dirichlet": "a univariate outcome (it is multivariate)",
                 "Binomial": "a regularised incomplete beta function", "BetaBinomial": "a regularised incomplete beta function",
                 "ZIPoisson": "a regularised incomplete gamma function"}


def predq_require(name):
    """NotImplementedError naming the family and what its predictive cdf would need (six families are built)."""
    if name not in PREDQ_FAMILIES:
        raise NotImplementedError("predictive cdf / quantiles of %s need %s, which is not built" % (name, PREDQ_MISSING.get(name, "?")))


def predictive_cdf_rows(name, y, m, v, gh_T=0, return_sf=False, device=None, **kw):
    """Per-row predictive cdf P(Y <= y_n) under q(f) = N(m_n, diag v_n) over the nodes of `log_predictive_density_rows`;
    return_sf=True: (cdf, sf), the survival function P(Y > y_n) summed on its own (a tail of 1e-200 keeps its digits).  y: (N,) --
    Ordinal labels, Weibull times.  Gaussian, HetGaussian, Bernoulli, Exponential, Ordinal, Weibull; the others InvalidArgument."""
    device = _resolve_device(device)
    y, m, v = _f64(y).reshape(-1), _f64(m), _f64(v)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    cdf = np.zeros(y.shape[0])
    sf = np.zeros(y.shape[0]) if return_sf else None
    check(lib.hmogp_predictive_cdf(device, LIK_IDS[name], lik_param(name, **kw), int(gh_T), y.shape[0], _p(y), _p(m), _p(v), _p(cdf),
                                   _p(sf) if return_sf else None))
    return (cdf, sf) if return_sf else cdf


def predictive_quantile_rows(name, m, v, probs, gh_T=0, device=None, **kw):
    """(N, len(probs)) predictive quantiles under q(f) = N(m_n, diag v_n): the y with cdf(y) = p; Bernoulli / Ordinal the
    smallest point of the support whose cdf is >= p.  A p outside (0, 1) gives a NaN column."""
    device = _resolve_device(device)
    m, v, probs = _f64(m), _f64(v), _f64(probs).reshape(-1)
    J = lik_dim_f(name, **kw)
    m, v = m.reshape(-1, J), v.reshape(-1, J)
    out = np.zeros((m.shape[0], probs.shape[0]))
    for c0 in range(0, max(probs.shape[0], 1), _lib.QUANT_MAXP):
        pc = np.ascontiguousarray(probs[c0:c0 + _lib.QUANT_MAXP])
        qc = np.zeros((m.shape[0], pc.shape[0]))
        check(lib.hmogp_predictive_quantile(device, LIK_IDS[name], lik_param(name, **kw), int(gh_T), m.shape[0], pc.shape[0], _p(pc),
                                            _p(m), _p(v), _p(qc)))
        out[:, c0:c0 + pc.shape[0]] = qc
    return out


def sample(name, F, seed=0, device=None, **kw):
    """One draw y ~ p(y | F[n]) per row on the device (the reference's `<likelihood>.samples`): returns (N, 1); (N, K) for
    Dirichlet.  Weibull: event times (N, 1), never censored.  Binomial, BetaBinomial: counts (N, 1) out of pred_trials trials."""
    device = _resolve_device(device)
    J = lik_dim_f(name, **kw)
    F = _f64(F).reshape(-1, J)
    Y = np.zeros((F.shape[0], 1 if name in _TWO_COLUMN_Y else lik_dim_y(name, **kw)))
    check(lib.hmogp_sample(device, LIK_IDS[name], lik_param(name, **kw), F.shape[0], int(seed) & (2 ** 64 - 1), _p(F), _p(Y)))
    return Y


def select_inducing_rows(X, variance, lengthscale, Mmax, tol=0.0, forced=None, return_factor=False, device=None):
    """Inducing inputs chosen from the rows of X by greedy conditional variance = pivoted incomplete Cholesky of K_ff under the sum
    kernel k = sum_q variance[q] exp(-r_q^2 / 2) (`hmogp_select_inducing`).  X (N, P); variance, lengthscale: Q values each;
    `forced`: rows that are picked first, in that order.  Returns a dict: Mout, pivots (Mout,) int64, Z (Mout, P), dpiv (Mout,) = d at
    each pick (its root is the Cholesky diagonal of K_uu in pick order), trace (Mout + 1,) = tr(K_ff - Q_ff) before each pick and after
    the last; with return_factor also L (N, Mmax) (columns at Mout and beyond are zero) and the final d (N,)."""
    device = _resolve_device(device)
    X = _f64(X)
    X = X.reshape(X.shape[0], -1) if X.ndim != 2 else X
    N, P = X.shape
    var, ell = _f64(np.atleast_1d(variance)).ravel(), _f64(np.atleast_1d(lengthscale)).ravel()
    if var.shape != ell.shape:
        raise _lib.InvalidArgument("select_inducing_rows: variance and lengthscale must have one entry per kernel each")
    Mmax = int(Mmax)
    fo = np.zeros(0, dtype=np.int64) if forced is None else np.ascontiguousarray(np.ravel(forced), dtype=np.int64)
    Ma = max(Mmax, 1)
    pivots, Z, dpiv, trace = np.zeros(Ma, dtype=np.int64), np.zeros((Ma, max(P, 1))), np.zeros(Ma), np.zeros(Ma + 1)
    L = np.zeros((max(N, 1), Ma)) if return_factor else None
    d = np.zeros(max(N, 1)) if return_factor else None
    Mout = C.c_int32(0)
    check(lib.hmogp_select_inducing(device, N, P, _p(X), var.shape[0], _p(var), _p(ell), Mmax, float(tol), fo.shape[0],
                                    fo.ctypes.data_as(_lib.c_int64_p) if fo.shape[0] else None, pivots.ctypes.data_as(_lib.c_int64_p),
                                    _p(Z), _p(dpiv), _p(trace), _p(L) if return_factor else None, _p(d) if return_factor else None,
                                    C.byref(Mout)))
    M = int(Mout.value)
    out = dict(Mout=M, pivots=pivots[:M].copy(), Z=Z[:M].copy(), dpiv=dpiv[:M].copy(), trace=trace[:M + 1].copy())
    if return_factor:
        out.update(L=L, d=d)
    return out


def qf_input_grad_rows(X, Z, variance, lengthscale, a, C, W, exact=True, device=None):
    """Gradients of q(f) with respect to the inputs, from explicit coefficients (`hmogp_qf_input_grad`).  X (N, P); Z (M, Q P)
    laid out as the engine's Z (latent q's inducing inputs in columns q P .. q P + P); variance, lengthscale (Q,); a (Q, M); C (Q, M, M);
    W (Q, Df).  With k_qm = variance_q exp(-|x - z_qm|^2 / 2 l_q^2), p_q = sum_m a_qm k_qm, c_q = sum_mm' k_qm C_q,mm' k_qm',
    m_d = sum_q W_qd p_q and v_d = const + sum_q W_qd^2 c_q: returns (dm, dv), both (N, Df, P), dm[i, d, j] = d m_d / d x_j and
    dv[i, d, j] = d v_d / d x_j (of the signed v: no abs anywhere).  exact: the rounding variant of `rbf_cross_cov`.  A row's result
    depends on that row alone, bit for bit."""
    device = _resolve_device(device)
    X = _f64(X)
    X = X.reshape(X.shape[0], -1) if X.ndim != 2 else X
    N, P = X.shape
    var, ell = _f64(np.atleast_1d(variance)).ravel(), _f64(np.atleast_1d(lengthscale)).ravel()
    Q = var.shape[0]
    a, W = _f64(a), _f64(W)
    a = a.reshape(Q, -1) if a.ndim != 2 else a
    W = W.reshape(Q, -1) if W.ndim != 2 else W
    M, Df = a.shape[1], W.shape[1]
    Z, C_ = _f64(Z), _f64(C)
    if ell.shape != var.shape or a.shape[0] != Q or W.shape[0] != Q or Z.shape != (M, Q * P) or C_.shape != (Q, M, M):
        raise _lib.InvalidArgument("qf_input_grad_rows: shapes must be X (N, P), Z (M, Q P), variance / lengthscale (Q,), a (Q, M), "
                                   "C (Q, M, M), W (Q, Df)")
    dm, dv = np.zeros((N, Df, P)), np.zeros((N, Df, P))
    check(lib.hmogp_qf_input_grad(device, N, P, _p(X), M, Q, _p(Z), _p(var), _p(ell), 1 if exact else 0, _p(a), _p(C_), Df, _p(W),
                                  _p(dm), _p(dv)))
    return dm, dv
