"""`SVMOGP` -- the reference's model class (hetmogp/svmogp.py:16-217) on top of the HIP engine.

Same constructor, `log_likelihood()`, `parameters_changed()`, `set_data` / `new_batch` / `stochastic_grad` / `callback`,
same attributes (`q_u_means`, `q_u_chols`, `Z`, `kern_list`, `B_list`, `elbo`, `vem_step`, `ve_count`, `batch_scale`,
`posteriors`), same gradient gating.  Everything numerical happens in `libhetmogp_hip.so`; GPy / paramz / climin are
not dependencies: the small part of paramz the reference's drivers use (`optimizer_array`, `_grads`, `optimize`,
`model['regex'].fix()`) is provided here.  README of the reference calls the class `HetMOGP`; both names are exported.
"""
import numpy as np

from . import _lib
from . import util
from .engine import Engine, pinned_empty
from .param import Param, match, logexp_f, logexp_finv, logexp_gradfactor


class Posterior(object):
    """What `model.posteriors[q]` exposes to the reference's `_raw_predict` (svmogp.py:238-251)."""

    def __init__(self, mean, woodbury_vector, woodbury_inv):
        self.mean, self.woodbury_vector, self.woodbury_inv = mean, woodbury_vector, woodbury_inv


class DeviceAdadelta(object):
    """climin.Adadelta as `util.vem_algorithm` drives it (util.py:321-329: iteration protocol, `minimize_until`, info dict
    with 1-based `n_iter`), with q(u) -- 98 % of the optimiser vector -- and its accumulators resident in HBM
    (`hmogp_qu_load` / `hmogp_qu_adadelta`).  The few remaining free parameters (Z, variance, W, ...) follow the same
    recurrence here on the host, in the optimiser's (Logexp) coordinates.  One iteration = the reference's
    `stochastic_grad` (next contiguous minibatch, 4 E-steps then 1 M-step gating, svmogp.py:188-199) wrapped in the two
    halves of the Adadelta update.  Iterates are bit-identical to `util.Adadelta(model.optimizer_array,
    model.stochastic_grad, ...)`; `model.q_u_means` / `q_u_chols` are refreshed from the device when the loop ends
    (`finish()`), not after every iteration."""

    def __init__(self, model, step_rate=1.0, decay=0.9, momentum=0.0, offset=1e-4):
        self.model = model
        self.step_rate, self.decay, self.momentum, self.offset = step_rate, decay, momentum, offset
        self.small = [p for _, p in model._named_params()
                      if not p.is_fixed and p is not model.q_u_means and p is not model.q_u_chols]
        parts = [logexp_finv(p.values.ravel()) if p.positive else p.values.ravel().copy() for p in self.small]
        self.wrt = np.concatenate(parts) if parts else np.zeros(0)
        self.gms, self.sms, self.step = (np.zeros_like(self.wrt) for _ in range(3))
        self.n_iter = 0
        model._engine.qu_load(model.q_u_means.values, model.q_u_chols.values)
        model._qu_on_device = True

    def _set_small(self):
        i = 0
        for p in self.small:
            v = self.wrt[i:i + p.size].reshape(p.shape)
            p[...] = logexp_f(v) if p.positive else v
            i += p.size

    def _small_gradient(self):
        parts = []
        for p in self.small:
            g = np.asarray(p.gradient, dtype=float).ravel()
            parts.append(g * logexp_gradfactor(p.values.ravel()) if p.positive else g)
        return -np.concatenate(parts) if parts else np.zeros(0)

    def __iter__(self):
        m, eng = self.model, self.model._engine
        try:
            while True:
                d, o, mom, rate = self.decay, self.offset, self.momentum, self.step_rate
                step1 = self.step * mom                            # the operations of util.Adadelta, in its order
                self.wrt -= step1
                eng.qu_adadelta(0, rate, mom, d, o)
                m.set_data(*m.new_batch())                         # stochastic_grad, svmogp.py:188-199
                self._set_small()
                m.parameters_changed()
                g = self._small_gradient()
                if m.vem_step:
                    if m.ve_count > 2:
                        m.ve_count, m.vem_step = 0, False
                    else:
                        m.ve_count += 1
                else:
                    m.vem_step = True
                t1 = g * g
                t1 *= (1 - d)
                self.gms *= d
                self.gms += t1
                t1 = np.sqrt(self.sms + o)
                t1 /= np.sqrt(self.gms + o)
                t1 *= g
                t1 *= rate
                self.wrt -= t1
                self.step = step1 + t1
                t2 = self.step * self.step
                t2 *= (1 - d)
                self.sms *= d
                self.sms += t2
                eng.qu_adadelta(1, rate, mom, d, o)
                m._qu_host_stale = True                            # (refreshed on the next READ of m.q_u_means / q_u_chols)
                self.n_iter += 1
                yield dict(n_iter=self.n_iter, gradient=g, step=self.step)
        finally:
            try:
                self.finish()
            except Exception:      # interpreter shutdown with the generator still alive: nothing left to sync into
                pass

    def finish(self):
        """Bring q(u) back into the model's parameter arrays.  Like every other parameter it is left at the point of the
        LAST EVALUATION, which is what the reference's model object holds when its Adadelta loop ends (climin applies
        the second half-step to its own `wrt` only; the model is written by stochastic_grad, svmogp.py:188): the engine
        keeps that half-step pending (`hmogp_qu_adadelta`).  No re-evaluation here; the model is marked dirty."""
        m = self.model
        if getattr(m, "_qu_on_device", False):
            mu, L = m._engine.qu_read()
            m._qu_host_stale = False
            np.asarray(m._q_u_means)[...] = mu
            np.asarray(m._q_u_chols)[...] = L
            m._qu_on_device = False
            m._dirty = True

    def minimize_until(self, criterion):
        it = iter(self)
        try:
            for info in it:
                if criterion(info):
                    return info
        finally:
            it.close()


class DeviceNatGrad(DeviceAdadelta):
    """The SVI loop with the NATURAL-GRADIENT update of q(u) the north-star names (the reference has none: it feeds the
    Euclidean gradients of svmogp_inf.py:168-178 to Adadelta).  Same iteration protocol and 4 x E / 1 x M gating as
    DeviceAdadelta (svmogp.py:188-199); what differs is the E-step: q(u) -- resident in HBM -- takes
        S_q^-1 <- S_q^-1 - 2 gamma dL/dS_q ,  S_q^-1 m_q <- S_q^-1 m_q + gamma (dL/dm_q - 2 dL/dS_q m_q)
    on the device (`hmogp_qu_natgrad`: in place, no host copy of q(u)), the remaining free parameters keep their Adadelta
    recurrence on the host and only move on M-steps (their E-step gradients are gated to zero by the reference's own
    logic).  A step that would leave the positive-definite cone is retried with gamma halved (q(u) untouched by a failed
    step); `gamma_used` records the last accepted value.
    `overlap=True` (default; single-process models): the step is enqueued with `hmogp_qu_natgrad_async` -- committed on the device
    only if it stays inside the cone -- and the loop goes straight on to the next minibatch, whose upload, staging and K_uf
    construction run beside the step's factorisation chain; the outcome is read after that next evaluation.  The info dict of an
    E-step therefore carries `gamma=None, step_taken=None, pending=True, gamma_requested=<enqueued step size>` and
    `last_resolved = {gamma, step_taken}` of the most recent step whose outcome is known (None before the first); `ng.step_taken` /
    `ng.gamma_used` / `ng.rejected` follow with one E-step of delay.  A refused step is not retried on the spot (its gradients
    are gone, the minibatch is lost): the step size of the following E-steps is halved until one is accepted.  Callers that
    monitor gamma / step_taken per iteration as the synchronous loop allows pass `overlap=False`.  E-step evaluations also skip the
    gradient of q(u)'s factor (HMOGP_EVAL_NO_G_L: the update consumes dL/dS and dL/dm only)."""

    def __init__(self, model, gamma=0.1, step_rate=1.0, decay=0.9, momentum=0.0, offset=1e-4, gamma_start=1e-5, warmup=20,
                 overlap=True):
        DeviceAdadelta.__init__(self, model, step_rate=step_rate, decay=decay, momentum=momentum, offset=offset)
        self.overlap = bool(overlap) and getattr(model, "_dist", None) is None
        self._backoff = 1.0          # overlap mode: factor on the scheduled step size after refused steps (halved per refusal)
        self._pending = False
        self._n_resolved = 0         # overlap mode: steps whose outcome has been read back
        self.gamma = float(gamma)
        self.gamma_used = float(gamma)
        self.rejected = 0            # step sizes refused by hmogp_qu_natgrad (halved and retried)
        self.skipped = 0             # E-steps in which all eight retries were refused: q(u) unchanged, info["gamma"] == 0.0
        self.step_taken = True
        # Step-size schedule: log-linear from gamma_start to gamma over the first `warmup` E-steps.  With N >> M the data term
        # dominates the prior in the new precision, and then m_new = S_new theta_new is nearly the FULL Newton step of the mean
        # whatever gamma is (it cancels) -- from a poor start that overshoots for exp-link likelihoods (Poisson: measured ELBO
        # -1.2e7 -> -4.5e10 in one step of gamma = 0.1 at N_all = 1e6).  Only a gamma small enough for gamma * (data precision) to
        # be comparable with K_uu^-1 damps it; the schedule is the usual remedy for non-conjugate natural-gradient VI.
        self.gamma_start, self.warmup, self.e_steps = float(min(gamma_start, gamma)), int(warmup), 0

    def _resolve_pending(self, eng):
        """Outcome of the natural-gradient step that was enqueued in the previous E-step (overlap mode)."""
        taken = eng.qu_natgrad_status()
        self._pending = False
        self._n_resolved += 1
        self.step_taken = bool(taken)
        if taken:
            self.gamma_used, self._backoff = self._gam_pending, 1.0
        else:
            self.rejected += 1
            self.gamma_used = 0.0
            self._backoff *= 0.5
            if self._backoff < 2.0 ** -8:      # eight refusals in a row: say so (q(u) has not moved since) and start over
                self.skipped += 1
                self._backoff = 1.0
                import warnings
                warnings.warn("natural-gradient E-steps refused eight times in a row down to gamma = %.3g (q(u) unchanged)"
                              % (self._gam_pending,), RuntimeWarning)

    def __iter__(self):
        m, eng = self.model, self.model._engine
        self._pending = False
        try:
            while True:
                d, o, mom, rate = self.decay, self.offset, self.momentum, self.step_rate
                step1 = self.step * mom
                self.wrt -= step1
                m.set_data(*m.new_batch())                         # stochastic_grad, svmogp.py:188-199
                self._set_small()
                e_step = bool(m.vem_step)
                m._skip_g_L = e_step and m._dist is None           # (E-steps: dL/dS and dL/dm are all the update reads)
                try:
                    m.parameters_changed()                         # (a pending step completes on the device in front of it)
                finally:
                    m._skip_g_L = False
                if self._pending:
                    self._resolve_pending(eng)
                g = self._small_gradient()
                if m.vem_step:
                    if m.ve_count > 2:
                        m.ve_count, m.vem_step = 0, False
                    else:
                        m.ve_count += 1
                else:
                    m.vem_step = True
                t1 = g * g
                t1 *= (1 - d)
                self.gms *= d
                self.gms += t1
                t1 = np.sqrt(self.sms + o)
                t1 /= np.sqrt(self.gms + o)
                t1 *= g
                t1 *= rate
                self.wrt -= t1
                self.step = step1 + t1
                t2 = self.step * self.step
                t2 *= (1 - d)
                self.sms *= d
                self.sms += t2
                if e_step:                                          # the evaluation carried the q(u) group
                    frac = min(1.0, self.e_steps / float(self.warmup)) if self.warmup > 0 else 1.0
                    gam = float(np.exp(np.log(self.gamma_start) + frac * (np.log(self.gamma) - np.log(self.gamma_start))))
                    self.e_steps += 1
                    if self.overlap:
                        self._gam_pending = gam * self._backoff
                        eng.qu_natgrad_async(self._gam_pending)
                        self._pending = True
                        m._qu_host_stale = True
                        m._dirty = True
                        self.n_iter += 1
                        #  the outcome of THIS step is not known yet: gamma / step_taken are None while it is pending;
                        # `gamma_requested` is what was enqueued, `last_resolved` the most recent step whose outcome has been read
                        # (None before the first one) -- the synchronous loop's per-iteration meaning is kept by overlap=False
                        yield dict(n_iter=self.n_iter, gradient=g, step=self.step, gamma=None, step_taken=None, pending=True,
                                   gamma_requested=self._gam_pending,
                                   last_resolved=(dict(gamma=self.gamma_used, step_taken=bool(self.step_taken))
                                                  if self._n_resolved else None))
                        continue
                    self.step_taken = False
                    for _ in range(8):
                        try:
                            eng.qu_natgrad(gam)
                            self.gamma_used, self.step_taken = gam, True
                            break
                        except np.linalg.LinAlgError:
                            self.rejected += 1
                            gam *= 0.5
                    if not self.step_taken:      # eight halvings left the positive-definite cone every time: q(u) did NOT move
                        self.gamma_used = 0.0
                        self.skipped += 1
                        import warnings
                        warnings.warn("natural-gradient E-step %d skipped: every step size down to %.3g left the positive-definite "
                                      "cone (q(u) unchanged)" % (self.e_steps, gam * 2.0), RuntimeWarning)
                    m._qu_host_stale = True
                    m._dirty = True
                self.n_iter += 1
                yield dict(n_iter=self.n_iter, gradient=g, step=self.step, gamma=self.gamma_used,
                           step_taken=bool(self.step_taken) if e_step else None)
        finally:
            try:
                if self._pending:
                    self._resolve_pending(eng)
                self.finish()
            except Exception:
                pass


class SVMOGP(object):
    def __init__(self, X, Y, Z, kern_list, likelihood, Y_metadata, name="SVMOGP", batch_size=None, W_list=None,
                 device=None, chunk_rows=0, exact_zero_windows=False, distributed=False, quirks="reference",
                 gradients_of_fixed=False, strict_qf=None):
        """The reference's constructor (svmogp.py:17) plus engine options (no reference equivalent):
        device            HIP device ordinal; default: LOCAL_RANK when `distributed`, else 0
        distributed       one process per GPU inside an initialised torch.distributed group: rows are sharded over ranks
        exact_zero_windows  False (default: dense) | True | "auto": the opt-in mode that skips products with EXACT zeros of K_uf
                          (results unchanged).  "auto" turns it on where it can pay off -- 1-D inputs that are
                          sorted within every task (what the reference's own slicing assumes, util.py:52-72) and
                          M <= 8192; unsorted / multi-dimensional inputs stay dense (and even when it is on, the
                          device falls back to full ranges for rows that are not banded); M < 128 stays dense too
                          (nothing to skip at that size, and the small-model kernels need the dense layout)
        quirks            "reference" (default: reproduce the reference's results including its known deviations from the
                          exact gradient) | "exact" (true ELBO gradients) | an int mask of _lib.QUIRK_*
        strict_qf         None (default) | "auto" | True | False.  "auto": evaluate on the default (explicit-inverse) path; the first
                          evaluation the engine flags as ill-conditioned (hmogp_outputs.cond_est beyond what that path keeps within
                          element-wise 1e-5 of the reference) is REPEATED through the reference's solve-based forms
                          (svmogp_inf.py:214-218, :144-161; HMOGP_EVAL_STRICT_QF) and so are the following ones until the estimate
                          has fallen 10x below the threshold again: the reference's numbers also where GPy's jitter ladder is
                          taken (K_uu with l >> inducing spacing, e.g. the notebook's own lengthscale 0.05 on
                          linspace(0, 1, M >= 24)), the ~2x step time paid only while K_uu is ill-conditioned.
                          None = "auto", except with exact_zero_windows on (the two exclude each other in the engine): then
                          False, and the ill-conditioned warning says so.  True = every evaluation strict (HMOGP_CFG_STRICT_QF).
                          False = never (the rounds 1-5 default; a flagged evaluation warns once per model).
        gradients_of_fixed  batch mode only: also evaluate the gradient groups whose parameters are all fixed (the
                          reference always computes them and the optimiser never reads them); default off, which makes
                          the VE steps of `vem_algorithm` skip the hyper-parameter / Z path."""
        import os
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if distributed else 0
        self._device = int(device)
        from .engine import set_default_device
        set_default_device(self._device, from_model=True)   # stand-alone likelihood helpers follow the FIRST model / an explicit choice
        self.name = name
        self.gradients_of_fixed = bool(gradients_of_fixed)
        self.batch_size = batch_size
        self.kern_list = kern_list
        self.likelihood = likelihood
        self.Y_metadata = Y_metadata
        self.num_inducing = Z.shape[0]                                   # M
        self.num_latent_funcs = len(kern_list)                           # Q
        self.num_output_funcs = likelihood.num_output_functions(Y_metadata)
        if W_list is None:
            self.W_list, self.kappa_list = util.random_W_kappas(self.num_latent_funcs, self.num_output_funcs, rank=1)
        else:
            self.W_list = W_list
            _, self.kappa_list = util.random_W_kappas(self.num_latent_funcs, self.num_output_funcs, rank=1)

        self.Xmulti_all = [np.ascontiguousarray(x, dtype=float).reshape(x.shape[0], -1) for x in X]
        self._dim_y = [lik.get_metadata()[0] for lik in likelihood.likelihoods_list]   # columns of a task's Y (1; Dirichlet: K)
        self.Ymulti_all = [np.ascontiguousarray(y, dtype=float).reshape(-1, dy) for y, dy in zip(Y, self._dim_y)]
        T = len(self.Ymulti_all)
        self.Xdim = Z.shape[1]
        if isinstance(strict_qf, str) and strict_qf != "auto":
            raise ValueError("strict_qf must be None, False, True or 'auto'")
        if isinstance(exact_zero_windows, str):
            if exact_zero_windows != "auto":
                raise ValueError("exact_zero_windows must be False, True or 'auto'")
            # (an explicit strict_qf=True / "auto" wins over windows="auto": the engine has no windowed strict kernels)
            exact_zero_windows = bool(strict_qf in (None, False) and self.Xdim == 1 and 128 <= self.num_inducing <= 8192 and
                                      all(x.shape[0] < 2 or bool(np.all(np.diff(x[:, 0]) >= 0.0)) for x in self.Xmulti_all))
        self.exact_zero_windows = bool(exact_zero_windows)
        # The engine refuses strict q(f) together with exact-zero windows (decide_mode: HMOGP_E_INVALID).  An EXPLICIT request for
        # both fails here, at construction ("auto" used to construct, train, and raise at the first flagged evaluation);
        # the default (None) resolves to "auto" without windows and to False with them.
        if strict_qf is None:
            strict_qf = False if self.exact_zero_windows else "auto"
        elif self.exact_zero_windows and (strict_qf is True or strict_qf == "auto"):
            raise ValueError("strict_qf=%r and exact_zero_windows exclude each other (the solve-based forms have no windowed "
                             "kernels): choose one" % (strict_qf,))
        self._strict_auto = strict_qf == "auto"
        self._strict_now = False
        self.strict_switches = 0          # how often "auto" went from the default to the strict path
        self.strict_evaluations = 0       # evaluations that ran through the strict forms (either mode)
        self.evaluations = 0              # parameters_changed() calls (a repeated evaluation at a switch counts once)
        self.strict_qf = (strict_qf is True) or (not self._strict_auto and bool(strict_qf))
        strict_qf = self.strict_qf
        # likelihoods that learn their own parameters
        self._lik_learn = [(t, l) for t, l in enumerate(likelihood.likelihoods_list) if l.learnable_params()]
        self._lik_pushed = {}
        if self._lik_learn and distributed:
            raise NotImplementedError("learnable likelihood parameters in a row-sharded (distributed=True) model: the statistic "
                                      "bundle does not carry their gradient (DESIGN 9e)")
        self._engine = Engine(likelihood.specs(), self.num_latent_funcs, self.num_inducing, self.Xdim, device=device,
                              chunk_rows=chunk_rows, exact_zero_windows=exact_zero_windows, cache_kuu=True,
                              reuse_outputs=True, quirks=quirks, strict_qf=strict_qf,
                              small_path=not distributed)   # gradients arrive in engine-owned page-locked arrays, copied into
                                                    # the parameters' .gradient fields by parameters_changed()
        # (distributed: the fused small-model kernels are chosen from THIS rank's row count; ranks whose shares straddle the
        #  threshold would round the replicated M x M algebra differently and the device-resident q(u) replicas, which are never
        #  re-synchronised, would drift apart -- every rank therefore keeps the regular kernels.  ADVICE r4)
        if self._lik_learn:                       #  turned on once, here, if and only if a likelihood learns something
            self._engine.lik_grad_enable(True)
        self._engine.set_data(self.Xmulti_all, self.Ymulti_all)
        self._engine_has_full = True      # False while foreign data (set_data of arrays that are not row ranges) is resident
        # distributed=True (inside an initialised torch.distributed group, one process per GPU): the rows of every
        # evaluation are sharded over the ranks and the statistic bundle is all-reduced once (hetmogp_amd/dist.py); every
        # rank holds identical parameters and receives identical gradients.
        self._dist = None
        if distributed:
            import torch.distributed as tdist
            from . import dist as hdist
            if not tdist.is_initialized():
                raise RuntimeError("distributed=True needs an initialised torch.distributed process group")
            self._dist = (hdist, hdist.StatsReducer(self._engine, device=device), tdist.get_rank(), tdist.get_world_size())
        self._rows = [(0, x.shape[0]) for x in self.Xmulti_all]
        self._last_batch = None
        if batch_size is None:
            self.stochastic = False
            self.Xmulti, self.Ymulti = self.Xmulti_all, self.Ymulti_all
        else:
            self.stochastic = True                                         # contiguous slicers, svmogp.py:43-47
            self.slicer_list = [util.draw_mini_slices(x.shape[0], self.batch_size) for x in self.Xmulti_all]
            self.set_data(*self.new_batch())

        Ztiled = np.tile(Z, (1, self.num_latent_funcs))                   # svmogp.py:52
        # the three large parameters live in page-locked host memory: they reach the GPU by DMA without a staging copy
        self.Z = Param("inducing inputs", Ztiled, storage=pinned_empty(Ztiled.shape))
        _, self.B_list = util.LCM(input_dim=self.Xdim, output_dim=self.num_output_funcs, rank=1,
                                  kernels_list=self.kern_list, W_list=self.W_list, kappa_list=self.kappa_list)
        M, Q = self.num_inducing, self.num_latent_funcs
        self._qu_on_device = False                # True while a DeviceAdadelta loop owns q(u): see the q_u_means property
        self._qu_host_stale = False
        self.q_u_means = Param("m_u", 2.5 * np.random.randn(M, Q), storage=pinned_empty((M, Q)))   # svmogp.py:66-67
        r, c = np.tril_indices(M)
        chols = np.zeros((M * (M + 1) // 2, Q))
        chols[r == c, :] = 1.0                                             # triang_to_flat(identity), :68
        self.q_u_chols = Param("L_u", chols, storage=pinned_empty(chols.shape))
        self.vem_step = True                                               # True = VE step, False = VM step
        self.ve_count = 0
        self.elbo = np.zeros((1, 1))
        self._log_marginal_likelihood = np.zeros((1, 1))
        self.posteriors = None
        self.batch_scale = [1.0] * T
        self.forced_rung = None
        self.last = None
        self._dirty = False
        for _, prm in self._named_params():       # a direct write to any parameter marks the model dirty (paramz would
            prm.add_observer(self._mark_dirty)    # re-run parameters_changed() at once; here it happens lazily, on the
        self.parameters_changed()                 # next read of a derived quantity)

    def _mark_dirty(self, _param=None):
        self._dirty = True

    def touch(self):
        """Mark the model dirty after a write that went around the parameter objects (`p.values[...] = v`, `np.copyto`,
        `ufunc(out=p)`, a view from `np.asarray(p)`): paramz would have re-run parameters_changed() by itself; here the next
        read of `log_likelihood()`, a gradient or a prediction re-evaluates."""
        self._dirty = True

    # q(u) is an attribute of the reference's model (svmogp.py:66-69) that callbacks and predict calls may read at any time.
    # While a DeviceAdadelta loop owns it (hmogp_qu_*), the host arrays are refreshed from the device on READ -- as of the
    # last evaluation, which is what the reference's model holds between climin iterations -- instead of after every
    # iteration (a 12.6 MB copy at M = 1024, Q = 3, paid only by whoever looks).
    def _qu_read_through(self):
        if self._qu_on_device and self._qu_host_stale:
            self._qu_host_stale = False
            mu, L = self._engine.qu_read()
            np.asarray(self._q_u_means)[...] = mu
            np.asarray(self._q_u_chols)[...] = L

    @property
    def q_u_means(self):
        self._qu_read_through()
        return self._q_u_means

    @q_u_means.setter
    def q_u_means(self, p):
        self._q_u_means = p

    @property
    def q_u_chols(self):
        self._qu_read_through()
        return self._q_u_chols

    @q_u_chols.setter
    def q_u_chols(self, p):
        self._q_u_chols = p

    def _refresh(self):
        if self._dirty:
            self.parameters_changed()

    # ------------------------------------------------------------------------------------------ reference surface
    def log_likelihood(self):
        """svmogp.py:82-83: a (1,1) ndarray, as the reference returns it."""
        self._refresh()
        return self._log_marginal_likelihood

    def _construction_W(self):
        """The chain factors of svmogp.py:98,141,143,156 come from the construction-time `self.W_list` /
        `self.kappa_list`, the ELBO from the live B_list."""
        W0 = np.stack([np.ravel(w) for w in self.W_list])
        k0 = np.stack([np.ravel(k) for k in self.kappa_list])
        return W0, k0

    def parameters_changed(self):
        """svmogp.py:85-166 -- one call into the engine, then the same gated writes to the `.gradient` fields."""
        T = len(self.Ymulti_all)
        self.batch_scale = [float(self.Xmulti_all[t].shape[0]) / float(self.Xmulti[t].shape[0]) for t in range(T)]
        if self.stochastic:
            mask = _lib.GROUP_QU if self.vem_step else (_lib.GROUP_HYPER | _lib.GROUP_Z)
        else:
            mask = _lib.GROUP_ALL
            if not self.gradients_of_fixed:      # groups whose parameters are ALL fixed: nobody reads their gradients
                if self.q_u_means.is_fixed and self.q_u_chols.is_fixed:
                    mask &= ~_lib.GROUP_QU
                hyper = [k.variance for k in self.kern_list] + [k.lengthscale for k in self.kern_list] + \
                        [B.W for B in self.B_list] + [B.kappa for B in self.B_list]
                hyper += [p for _, l in self._lik_learn for _, p in l.learnable_params()]
                if all(h.is_fixed for h in hyper):
                    mask &= ~_lib.GROUP_HYPER
        if self.Z.is_fixed:
            mask &= ~_lib.GROUP_Z
        for t, l in self._lik_learn:             # values an optimiser moved since the last evaluation go to the engine first
            vals = l.engine_values()
            if self._lik_pushed.get(t) is None or not np.array_equal(vals, self._lik_pushed[t]):
                self._engine.set_lik_params(t, vals)
                self._lik_pushed[t] = vals.copy()
        W0, k0 = self._construction_W()
        evaluate = self._engine.elbo_grad
        if self._dist is not None:
            hdist, reducer, rank, world = self._dist
            evaluate = lambda **kw: hdist.sharded_elbo_grad(self._engine, reducer, rank, world, **kw)  # noqa: E731
        on_dev = self._qu_on_device
        args = dict(
            Z=self.Z.values, m_u=None if on_dev else self.q_u_means.values, L_flat=None if on_dev else self.q_u_chols.values,
            variance=[float(k.variance[0]) for k in self.kern_list],
            lengthscale=[float(k.lengthscale[0]) for k in self.kern_list],
            W=np.stack([np.ravel(B.W.values) for B in self.B_list]),
            kappa=np.stack([np.ravel(B.kappa.values) for B in self.B_list]), W0=W0, kappa0=k0,
            batch_scale=self.batch_scale, row_begin=[r[0] for r in self._rows], row_end=[r[1] for r in self._rows],
            forced_rung=self.forced_rung, group_mask=mask)
        if getattr(self, "_skip_g_L", False) and self._dist is None:
            args["skip_g_L"] = True              # (set by DeviceNatGrad around its E-step evaluations)
        out = evaluate(strict_qf=self._strict_now, **args)
        ran_strict = self.strict_qf or self._strict_now
        if self._strict_auto:
            if not self._strict_now and out.get("ill_conditioned"):
                out = evaluate(strict_qf=True, **args)  # the same parameters again, now through the reference's solve-based forms
                self._strict_now = True                 # (only once that evaluation has succeeded; every rank of a sharded
                self.strict_switches += 1               #  model sees the same replicated estimate and switches with the others)
                ran_strict = True
            elif self._strict_now and max(out["cond_est"]) < 50.0:
                self._strict_now = False                # well-conditioned again (10x below the flag's threshold): default path next time
        self.evaluations += 1
        self.strict_evaluations += int(bool(ran_strict))
        self.last = out
        if out.get("ill_conditioned") and not getattr(self, "_warned_ill", False):
            self._warned_ill = True      # (once per model; model.last["cond_est"] / ["ill_conditioned"] are there on every evaluation)
            import warnings
            warnings.warn("K_uu is ill-conditioned for the %s path (condition estimates %s, jitter rungs %s): its ELBO / gradients may "
                          "differ from the reference's by more than 1e-5 element-wise%s (DESIGN.md 6a)" % (
                              "strict q(f)" if (self.strict_qf or self._strict_now) else "default (explicit-inverse)",
                              ["%.1e" % c for c in out["cond_est"]], out["rungs"],
                              "" if (self.strict_qf or self._strict_now) else
                              ("; exact_zero_windows is on, which excludes the strict q(f) forms -- construct the model without it"
                               if self.exact_zero_windows else "; construct the model with strict_qf=True or 'auto'")),
                          RuntimeWarning)
        self._log_marginal_likelihood = np.array([[out["elbo"]]])
        if not on_dev:                            # (device-resident q(u): its gradient stays in HBM for the optimiser)
            self.q_u_means.gradient = out["g_m_u"]
            self.q_u_chols.gradient = out["g_L_u"]
        for q, (k, B) in enumerate(zip(self.kern_list, self.B_list)):
            k.gradient = [out["g_variance"][q], out["g_lengthscale"][q]]
            B.gradient = np.hstack([out["g_W"][q], out["g_kappa"][q]])
        if not self.Z.is_fixed:
            self.Z.gradient = out["g_Z"]
        for t, l in self._lik_learn:             # gated with the hyper-parameters (zeros otherwise); read after a strict re-evaluation
            l.set_engine_gradient(self._engine.lik_grad(t))
        self.posteriors = None                                               # built lazily (prediction only)
        self._dirty = False

    def set_data(self, X, Y):
        """svmogp.py:168-173.  Batches produced by `new_batch()` are row ranges of the data already in HBM; anything
        else is uploaded."""
        if self._last_batch is not None and X is self._last_batch[0] and Y is self._last_batch[1]:
            if not self._engine_has_full:        # foreign data was uploaded in between: the row ranges refer to the
                self._engine.set_data(self.Xmulti_all, self.Ymulti_all)   # full data set, put it back first
                self._engine_has_full = True
            self._rows = list(self._last_batch[2])
        else:
            Xc = [np.ascontiguousarray(x, dtype=float).reshape(x.shape[0], -1) for x in X]
            Yc = [np.ascontiguousarray(y, dtype=float).reshape(-1, dy) for y, dy in zip(Y, self._dim_y)]
            self._engine.set_data(Xc, Yc)
            self._engine_has_full = False
            self._rows = [(0, x.shape[0]) for x in Xc]
            X, Y = Xc, Yc
        self.Xmulti, self.Ymulti = X, Y


    def init_q_u_to_prior(self):
        """q(u_q) := p(u_q) = N(0, K_uu,q) (L_q = jitchol(K_uu,q), m_q = 0; covariance and factorisation on the device:
        hmogp_rbf_cross_cov + hmogp_jitchol_inv, GPy's jitter ladder if K_uu needs it).  Not in the reference, whose
        constructor starts from S_q = I (svmogp.py:66-69): with many close inducing points K_uu^-1 S K_uu^-1 is then
        enormous, q(f) has variances of 1e3 and more, and the expectations of exp-link likelihoods (Poisson, Gamma) are
        astronomically large -- a natural-gradient (Newton-like) step computed from them diverges.  Adadelta's small
        Euclidean steps survive that start; the natural-gradient loop starts from the prior instead."""
        from .engine import jitchol_inv
        dev = self._engine_device()
        r, c = np.tril_indices(self.num_inducing)
        K = np.stack([k.K(self.Z.values[:, q * self.Xdim:(q + 1) * self.Xdim]) for q, k in enumerate(self.kern_list)])
        L, _, _ = jitchol_inv(0.5 * (K + K.transpose(0, 2, 1)), device=dev)
        for q in range(self.num_latent_funcs):
            self.q_u_chols[:, q] = L[q][r, c]
        self.q_u_means[...] = 0.0
        self._dirty = True
        return self

    def shuffle_rows(self, seed=0):
        """Permute the rows of every task ONCE (data resident in HBM are re-uploaded in the new order), so that the contiguous
        minibatch slices of `new_batch` (the reference's protocol, util.py:52-72: slices are visited in order and never shuffled)
        become uniform random subsets.  Not in the reference.  `model.Xmulti_all` / `Ymulti_all` ARE reordered (user code that indexes
        them afterwards sees the new order); `model.row_permutation[t]` maps the new rows to the original ones.  Needed by natural-gradient SVI: a contiguous slice of sorted
        inputs informs a small part of the input space only, its batch_scale pretends the whole data set looks like it, and a
        natural-gradient step towards that local, over-confident posterior diverges where Adadelta's tiny Euclidean steps do
        not (measured at N_all = 1e6, batch 8192: ELBO -3e7 -> -1e17 within two steps at gamma = 0.1)."""
        if self.exact_zero_windows:
            import warnings
            warnings.warn("shuffle_rows() with exact_zero_windows on: the windows mode skips exact zeros of K_uf for SORTED rows; "
                          "after the shuffle every minibatch is unbanded and the device falls back to full ranges (results "
                          "unchanged, the mode only adds overhead)", RuntimeWarning)
        rng = np.random.RandomState(seed)
        prev = getattr(self, "row_permutation", None)
        self.row_permutation = []    # row_permutation[t][i] = index in the ORIGINAL Xmulti_all[t] of what is now row i (composes)
        for t in range(len(self.Ymulti_all)):
            perm = rng.permutation(self.Xmulti_all[t].shape[0])
            self.row_permutation.append(perm if prev is None else prev[t][perm])
            self.Xmulti_all[t] = np.ascontiguousarray(self.Xmulti_all[t][perm])
            self.Ymulti_all[t] = np.ascontiguousarray(self.Ymulti_all[t][perm])
        self._engine.set_data(self.Xmulti_all, self.Ymulti_all)
        self._engine_has_full = True
        self._last_batch = None
        if self.stochastic:
            self.set_data(*self.new_batch())
        else:
            self.Xmulti, self.Ymulti = self.Xmulti_all, self.Ymulti_all
            self._rows = [(0, x.shape[0]) for x in self.Xmulti_all]
        self._dirty = True
        return self

    def new_batch(self):
        """svmogp.py:175-186: the next contiguous slice of every task."""
        Xb, Yb, rows = [], [], []
        for t in range(len(self.Ymulti_all)):
            sl = next(self.slicer_list[t])
            n = self.Xmulti_all[t].shape[0]
            rows.append((min(sl.start, n), min(sl.stop, n)))
            Xb.append(self.Xmulti_all[t][sl])
            Yb.append(self.Ymulti_all[t][sl])
        self._last_batch = (Xb, Yb, rows)
        return Xb, Yb

    def stochastic_grad(self, parameters):
        """svmogp.py:188-199: 4 consecutive E-step gradients, then 1 M-step gradient."""
        self.set_data(*self.new_batch())
        g = self._grads(parameters)
        if self.vem_step:
            if self.ve_count > 2:
                self.ve_count = 0
                self.vem_step = False
            else:
                self.ve_count += 1
        else:
            self.vem_step = True
        return g

    def device_adadelta(self, step_rate=1.0, decay=0.9, momentum=0.0, offset=1e-4):
        """An Adadelta optimiser over `stochastic_grad` with q(u) and its accumulators resident in HBM (DeviceAdadelta),
        or None when that does not apply (batch mode, q(u) fixed) -- callers then fall back to
        `util.Adadelta(model.optimizer_array, model.stochastic_grad, ...)`, which produces the same iterates.
        [r4] Also in a row-sharded (distributed=True) model: every rank holds the same resident q(u), the all-reduced bundle gives
        every rank the same gradients, and the device recurrence is deterministic -- the replicas stay bit-identical."""
        if not self.stochastic or self.q_u_means.is_fixed or self.q_u_chols.is_fixed:
            return None
        return DeviceAdadelta(self, step_rate=step_rate, decay=decay, momentum=momentum, offset=offset)

    def device_natgrad(self, gamma=0.1, step_rate=1.0, decay=0.9, momentum=0.0, offset=1e-4, shuffle=True, seed=0,
                       init="prior", overlap=True):
        """The SVI loop with natural-gradient E-steps on the device-resident q(u) (DeviceNatGrad); None when it does not
        apply (same conditions as `device_adadelta`).  `shuffle` (default on): `shuffle_rows(seed)` first -- natural-gradient
        steps need minibatches that represent the whole data set.  `init="prior"` (default) starts q(u) at p(u)
        (`init_q_u_to_prior`); None keeps the model's current q(u).  `overlap=True` (default since round 5) enqueues the E-step's
        update and reads its outcome one evaluation later: the yielded info has `gamma=None, step_taken=None, pending=True` for
        that step (see DeviceNatGrad); pass `overlap=False` for the synchronous loop's per-iteration `gamma` / `step_taken`."""
        if not self.stochastic or self.q_u_means.is_fixed or self.q_u_chols.is_fixed:
            return None
        if shuffle:                 # (distributed: every rank holds all rows and the same seed gives the same permutation)
            self.shuffle_rows(seed)
        if init == "prior":      # see init_q_u_to_prior: the reference's S = I start is no place to take Newton-like steps from
            self.init_q_u_to_prior()
        elif init is not None:
            raise ValueError("init must be 'prior' or None")
        return DeviceNatGrad(self, gamma=gamma, step_rate=step_rate, decay=decay, momentum=momentum, offset=offset, overlap=overlap)

    def callback(self, i, max_iter, verbose=True, verbose_plot=False):
        """svmogp.py:201-217."""
        self.elbo[i["n_iter"] - 1, 0] = float(self.log_likelihood()[0, 0])
        if verbose and i["n_iter"] % 50 == 0:
            print("svi - iteration " + str(i["n_iter"]) + "/" + str(int(max_iter)))
        return i["n_iter"] > max_iter

    # ------------------------------------------------------------------------------------------ paramz-like view
    def _named_params(self):
        """Link order of svmogp.py:71-75: Z (index 0), m_u, L_u, kernels (variance, lengthscale), B_q (W, kappa)."""
        out = [("%s.inducing_inputs" % self.name, self.Z), ("%s.m_u" % self.name, self.q_u_means),
               ("%s.L_u" % self.name, self.q_u_chols)]
        for q, k in enumerate(self.kern_list):
            out += [("%s.kern_q%d.variance" % (self.name, q), k.variance), ("%s.kern_q%d.lengthscale" % (self.name, q), k.lengthscale)]
        for q, B in enumerate(self.B_list):
            out += [("%s.B_q%d.W" % (self.name, q), B.W), ("%s.B_q%d.kappa" % (self.name, q), B.kappa)]
        for t, l in getattr(self, "_lik_learn", ()):       # last: the layout of a model without them does not move
            out += [("likelihood.%d.%s" % (t, n), p) for n, p in l.learnable_params()]
        return out

    def __getitem__(self, pattern):
        return match(self._named_params(), pattern)

    @property
    def optimizer_array(self):
        """Free parameters, positive ones through paramz's Logexp inverse.  The returned array is a persistent buffer
        (optimisers such as Adadelta update it in place, util.py:327)."""
        parts = [logexp_finv(p.values.ravel()) if p.positive else p.values.ravel() for _, p in self._named_params() if not p.is_fixed]
        x = np.concatenate(parts) if parts else np.zeros(0)
        if getattr(self, "_opt_buf", None) is None or self._opt_buf.shape != x.shape:
            self._opt_buf = x.copy()
        else:
            self._opt_buf[...] = x
        return self._opt_buf

    def _free_plan(self):
        """(params, indices of the positive entries of the optimiser vector) of the free parameters, rebuilt when a fix() /
        unfix() changes the set: the transforms below then touch ONLY the few positive entries (variance, lengthscale, kappa), once,
        by index -- not once per parameter (an objective evaluation of a notebook-sized model takes 0.2 ms on the device: per-
        parameter NumPy calls were a third of the wall time) and not over the whole vector either (1.6 M entries, almost all
        q(u), at M = 1024: expm1 / log1p over all of them cost ~90 ms per L-BFGS evaluation and overflowed on very negative
        unconstrained entries)."""
        params = [p for _, p in self._named_params()]
        sig = tuple((id(p), p.is_fixed, p.size) for p in params)
        plan = getattr(self, "_plan", None)
        if plan is None or plan[0] != sig:
            free = [p for p in params if not p.is_fixed]
            mask = np.concatenate([np.full(p.size, bool(p.positive)) for p in free]) if free else np.zeros(0, bool)
            idx = np.flatnonzero(mask)
            plan = self._plan = (sig, free, idx, bool(idx.size))
        return plan

    @optimizer_array.setter
    def optimizer_array(self, x):
        x = np.asarray(x, dtype=float)
        _, free, idx, any_pos = self._free_plan()
        vals = x
        if any_pos:
            vals = x.copy()
            vals[idx] = logexp_f(x[idx])
        i = 0
        for p in free:
            n = p.size
            np.ndarray.__setitem__(p, Ellipsis, vals[i:i + n].reshape(p.shape))   # (no per-parameter notification: ...
            i += n
        self.parameters_changed()                                                  # ... one evaluation for the whole vector)

    def _transformed_gradient(self):
        _, free, idx, any_pos = self._free_plan()
        if not free:
            return np.zeros(0)
        g = np.concatenate([np.asarray(p.gradient, dtype=float).ravel() for p in free])
        if any_pos:
            theta = np.concatenate([p.values.ravel() for p in free if p.positive])
            g[idx] *= logexp_gradfactor(theta)
        return g

    def _grads(self, x):
        """paramz Model._grads: set the optimiser vector (fires parameters_changed) and return the gradient of the
        OBJECTIVE (- log likelihood)."""
        self.optimizer_array = x
        return -self._transformed_gradient()

    MAX_CONSECUTIVE_FAILURES = 25

    def objective_function(self):
        return -float(self._log_marginal_likelihood[0, 0])

    def optimize(self, messages=False, max_iters=100, **kw):
        """paramz Model.optimize default: scipy L-BFGS-B on (objective, gradient) over the free parameters.  Like paramz's
        `_objective_grads`, a failed evaluation (LinAlgError from the jitter ladder, the 'Sqi' ValueError, a non-finite
        ELBO) returns an infinite objective so that the line search backs off instead of aborting; an evaluation that
        reports v < 0 (the reference only prints 'v negative!', svmogp_inf.py:221, and carries on with a meaningless
        ELBO) is treated the same way.  The parameters of the best finite evaluation are restored at the end."""
        from scipy.optimize import minimize
        best = {"f": np.inf, "x": None}
        failures = [0]

        def f(x):
            try:
                g = self._grads(x)
                obj = self.objective_function()
                bad = (not np.isfinite(obj)) or bool(self.last and self.last.get("v_negative"))
            except _lib.InvalidArgument:
                raise                             # a programming / ABI error, not a failed evaluation
            except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
                g, obj, bad = np.zeros_like(x), np.inf, True
            if bad:
                failures[0] += 1
                if failures[0] > self.MAX_CONSECUTIVE_FAILURES:
                    raise RuntimeError("SVMOGP.optimize: %d consecutive failed evaluations" % failures[0])
                return np.inf, np.clip(np.nan_to_num(g), -1e10, 1e10)
            failures[0] = 0
            if obj < best["f"]:
                best["f"], best["x"] = obj, np.array(x, copy=True)
            return obj, g

        x0 = self.optimizer_array.copy()
        if x0.size == 0:
            return self
        res = minimize(f, x0, jac=True, method="L-BFGS-B", options={"maxiter": int(max_iters), "maxfun": int(max_iters),
                                                                   "disp": bool(messages)})
        self.optimizer_array = best["x"] if best["x"] is not None else res.x
        return self

    # ------------------------------------------------------------------------------------------ prediction
    def _ensure_posteriors(self):
        self._refresh()
        if self.posteriors is None:
            wv, wi = self._engine.posterior_u()
            self.posteriors = [Posterior(self.q_u_means.values[:, q:q + 1], wv[q][:, None], wi[q])
                               for q in range(self.num_latent_funcs)]
        return self.posteriors

    REFERENCE_ROUTE_MAX_ROWS = 8192      # `_raw_predict_f` factorises the N x N K_ff of a task's training inputs

    def _raw_predict(self, Xnew, latent_function_ind=None, full_cov=False, kern=None, route="default"):
        """svmogp.py:219-253: posterior of the latent u_q at Xnew (mean, |variance|).  route="reference" reproduces
        `kern.K(self.Z, Xnew)` under GPy's input slicing, which hands the kernel the FIRST P columns of the M x (Q P)
        inducing array -- latent 0's block whatever q is; the default uses block q (the two agree while Z is the tiled
        initialisation of svmogp.py:52, i.e. always when Z is fixed)."""
        q = 0 if latent_function_ind is None else latent_function_ind
        kern = self.kern_list[q] if kern is None else kern
        post = self._ensure_posteriors()[q]
        b = 0 if route == "reference" else q
        Zq = self.Z.values[:, b * self.Xdim:(b + 1) * self.Xdim]
        from .engine import gemm
        dev = self._engine_device()
        Kx = kern.K(Zq, np.asarray(Xnew, dtype=float).reshape(-1, self.Xdim))       # on the device (hmogp_rbf_cross_cov)
        wv = np.asarray(post.woodbury_vector, dtype=float).reshape(Kx.shape[0], -1)
        mu = gemm(Kx, wv, transA=True, device=dev)                                  # every product: hmogp_gemm_f64 (FP64 MFMA)
        WK = gemm(np.asarray(post.woodbury_inv, dtype=float), Kx, device=dev)
        if full_cov:
            var = kern.K(Xnew) - gemm(Kx, WK, transA=True, device=dev)
        else:
            var = (kern.Kdiag(Xnew) - np.sum(WK * Kx, 0))[:, None]
        return mu, np.abs(var)

    def predictive_new(self, Xnew, output_function_ind=None, kern_list=None):
        """svmogp.py:280-306: algebraically (m_fd(Xnew), |v_fd(Xnew)|) of calculate_q_f -- computed on the device."""
        d = 0 if output_function_ind is None else output_function_ind
        self._refresh()
        m, v = self._engine.predict_f(np.asarray(Xnew, dtype=float).reshape(-1, self.Xdim))
        return m[:, d:d + 1], np.abs(v[:, d:d + 1])

    def predict_f(self, Xnew, full_cov=False, functions=None):
        """q(f_d) at Xnew for every function d: (mean [N, Df], variance [N, Df]).  full_cov=True (GPy's `predict(full_cov=True)`;
        DESIGN 9r): the JOINT posterior of the functions `functions` (None: all) -- (mean [N, nD], cov [nD, N, nD, N]), cov[j, i, j', i'] =
        cov(f_dj(x_i), f_dj'(x_i')), exactly symmetric, its diagonal the variance above before any abs; nD * N <= 8192."""
        self._refresh()
        Xnew = np.asarray(Xnew, dtype=float).reshape(-1, self.Xdim)
        if not full_cov:
            if functions is not None:
                raise ValueError("predict_f: `functions` selects the functions of the joint posterior (full_cov=True)")
            return self._engine.predict_f(Xnew)
        mean, cov = self._engine.predict_f_joint(Xnew, functions)
        return np.ascontiguousarray(mean.T), cov

    def _grad_functions(self, functions):
        if functions is None:
            return list(range(self.num_output_funcs))
        d = [int(f) for f in np.ravel(functions)]
        if any(f < 0 or f >= self.num_output_funcs for f in d):
            raise ValueError("functions: indices must lie in 0 .. %d" % (self.num_output_funcs - 1))
        return d

    def predictive_gradients(self, Xnew, functions=None):
        """Gradients of q(f) with respect to the inputs (GPy's `predictive_gradients`, at the level of the latent parameter functions;
        DESIGN 9t): (dm (N, nD, P), dv (N, nD, P)), dm[i, j, p] = d m_d / d x_p and dv[i, j, p] = d v_d / d x_p of function d =
        functions[j] at row i -- the local effect of input p on, e.g., a Poisson task's log-rate or a Bernoulli task's logit.
        functions=None: all Df functions; a list selects and orders them.  v is the SIGNED variance the engine's `predict_f` returns:
        the gradient is taken before any abs (`predictive_new` applies one)."""
        self._refresh()
        d = self._grad_functions(functions)
        dm, dv = self._engine.predict_f_grad(np.asarray(Xnew, dtype=float).reshape(-1, self.Xdim))
        return np.ascontiguousarray(dm[:, d, :]), np.ascontiguousarray(dv[:, d, :])

    def input_sensitivity(self, X=None, functions=None):
        """Relevance of every input dimension for every function (the kernels are isotropic: there are no ARD lengthscales to read):
        (nD, P), the root mean square over the rows of X of d m_d / d x_p (`predictive_gradients`).  X=None: the model's pooled training
        inputs of all tasks."""
        if X is None:
            X = np.concatenate(self.Xmulti_all, 0)
        dm, _ = self.predictive_gradients(X, functions)
        return np.sqrt(np.mean(dm * dm, axis=0))

    def _joint_seed(self, seed):
        if seed is None:       # (as `_Lik.samples`: one draw from NumPy's GLOBAL generator)
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        return int(seed)

    def sample_paths(self, size=10, functions=None, num_features=1024, seed=None):
        """`size` posterior sample paths of the functions `functions` (None: all) as FUNCTIONS (pathwise conditioning): a
        `PosteriorPaths` that can be evaluated at any inputs, any number of times -- the same draw on every call, no bound on N.  The
        prior part is `num_features` random Fourier frequencies per latent; the update through the inducing variables is exact.  A
        snapshot of the model as it is now.  seed=None draws the seed from NumPy's global generator."""
        self._refresh()
        return PosteriorPaths(self, size, functions, num_features, self._joint_seed(seed))

    def posterior_samples_f(self, Xnew, size=10, functions=None, seed=None, method="joint", num_features=1024):
        """`size` sample paths of the functions `functions` (None: all) at Xnew, drawn JOINTLY over functions and inputs from the
        posterior of `predict_f(full_cov=True)` (GPy's `posterior_samples_f`): (size, N, nD).  Draw s depends on (seed, s)
        only, not on `size`; seed=None draws the seed from NumPy's global generator.  method="pathwise" (DESIGN 9v): a temporary
        `sample_paths` set of `num_features` frequencies evaluated at Xnew -- no bound on nD * N."""
        if method == "pathwise":
            with self.sample_paths(size=size, functions=functions, num_features=num_features, seed=seed) as paths:
                return paths(Xnew)
        if method != "joint":
            raise ValueError("method must be 'joint' or 'pathwise'")
        self._refresh()
        F = self._engine.sample_f_joint(np.asarray(Xnew, dtype=float).reshape(-1, self.Xdim), functions, size=size,
                                        seed=self._joint_seed(seed))
        return np.ascontiguousarray(np.transpose(F, (0, 2, 1)))

    def posterior_samples(self, Xnew, task, size=10, seed=None, method="joint", num_features=1024):
        """`size` draws of task `task`'s output at Xnew (GPy's `posterior_samples`): the task's functions are drawn jointly
        (`posterior_samples_f`, by `method`), each draw is then pushed through the likelihood's sampler on the device (`hmogp_sample`,
        keyed by seed + 1 and the row s N + i).  (size, N); (size, N, K) for Dirichlet."""
        t = int(task)
        lik = self.likelihood.likelihoods_list[t]
        cols = [d for d in range(self.num_output_funcs) if self.Y_metadata["function_index"].flatten()[d] == t]
        seed = self._joint_seed(seed)
        if method == "joint":
            F = self.posterior_samples_f(Xnew, size=size, functions=cols, seed=seed)
        else:
            F = self.posterior_samples_f(Xnew, size=size, functions=cols, seed=seed, method=method, num_features=num_features)
        S, N, J = F.shape
        Y = np.asarray(lik.samples(F.reshape(S * N, J), seed=seed + 1))        # one launch: row s N + i is draw s at input i
        return Y.reshape(S, N, -1) if lik.name == "Dirichlet" else Y.reshape(S, N)

    def _raw_predict_f(self, Xnew, output_function_ind=None, kern_list=None):
        """svmogp.py:255-278, the route the reference's `predictive` / `negative_log_predictive` take: q(f_d) at the TRAINING
        inputs of d's task (mean m_fd, full covariance S_fd, svmogp_inf.py:43-51) becomes a GPy `Posterior` -- an N x N
        jitchol of K_ff -- and is regressed onto Xnew:  mu = K_x^T K_ff^-1 m_fd,  var = |diag K_xx - diag(K_x^T K_ff^-1 (K_ff -
        S_fd) K_ff^-1 K_x)|.  O(N^3) time and O(N^2) memory, so it is limited to REFERENCE_ROUTE_MAX_ROWS training rows per
        task.  It is a DIFFERENT estimator than `predictive_new` / `predict_f` (calculate_q_f at the new inputs): the two
        agree only where q(f) at the training inputs determines q(f) at Xnew.  All products, the factorisation (GPy's
        jitter ladder) and the covariances run on the device through the C-ABI building blocks; with
        K_ff - S_fd = sum_q W_q[d]^2 K^_q (Kuu^-1 - Kuu^-1 S_q Kuu^-1) K^_q^T nothing but `woodbury_inv` of q(u) is needed."""
        from .engine import rbf_cross_cov, gemm, jitchol_inv
        d = 0 if output_function_ind is None else output_function_ind
        kern_list = self.kern_list if kern_list is None else kern_list
        t = int(self.Y_metadata["function_index"].flatten()[d])
        X = self.Xmulti_all[t]
        N, P = X.shape[0], self.Xdim
        if N > self.REFERENCE_ROUTE_MAX_ROWS:
            raise ValueError("_raw_predict_f factorises the %d x %d K_ff of task %d (svmogp.py:255-278): limited to %d rows; use "
                             "predict_f / predictive_new / predictive(route='default')" % (N, N, t, self.REFERENCE_ROUTE_MAX_ROWS))
        Xnew = np.asarray(Xnew, dtype=float).reshape(-1, P)
        posts = self._ensure_posteriors()
        dev = self._engine_device()
        Kff, Dm, m = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, 1))
        Kx, Kxx = np.zeros((N, Xnew.shape[0])), np.zeros(Xnew.shape[0])
        for q, (kern, B) in enumerate(zip(kern_list, self.B_list)):
            w = float(np.ravel(B.W.values)[d])
            Bdd = w * w + float(np.ravel(B.kappa.values)[d])
            var, ell = float(kern.variance[0]), float(kern.lengthscale[0])
            Zq = self.Z.values[:, q * P:(q + 1) * P]
            Kq = rbf_cross_cov(X, Zq, var, ell, device=dev)                        # k_q(X, Z_q), GPy rounding order
            Kff += Bdd * rbf_cross_cov(X, X, var, ell, device=dev)                 # util.py:166-179
            m += w * gemm(Kq, posts[q].woodbury_vector, device=dev)                # m_fd = sum_q w K^ Kuu^-1 m_q
            Dm += (w * w) * gemm(gemm(Kq, posts[q].woodbury_inv, device=dev), Kq, transB=True, device=dev)
            Kx += Bdd * rbf_cross_cov(X, Xnew, var, ell, device=dev)
            Kxx += Bdd * var
        _, Kffi, rung = jitchol_inv(Kff[None], device=dev)                         # GPy Posterior.K_chol = jitchol(K)
        self.last_predict_rung = rung[0]
        wv = gemm(Kffi[0], m, device=dev)                                          # woodbury_vector = K_ff^-1 m_fd
        wi = gemm(gemm(Kffi[0], Dm, device=dev), Kffi[0], device=dev)              # woodbury_inv
        mu = gemm(Kx, wv, transA=True, device=dev)
        var = (Kxx - np.sum(gemm(wi, Kx, device=dev) * Kx, 0))[:, None]
        return mu, np.abs(var)

    _raw_predict_stochastic = _raw_predict_f                                       # svmogp.py:308-331: the same code

    def _engine_device(self):
        return getattr(self, "_device", 0)

    def _predict_route(self, X_t, t, route):
        """(m, |v|) of the functions of task t at X_t: [N, dim_f(t)]."""
        cols = [d for d in range(self.num_output_funcs) if self.Y_metadata["function_index"].flatten()[d] == t]
        if route == "reference":
            mv = [self._raw_predict_f(X_t, output_function_ind=d) for d in cols]
            return np.hstack([a for a, _ in mv]), np.hstack([b for _, b in mv])
        if route != "default":
            raise ValueError("route must be 'default' or 'reference'")
        m, v = self.predict_f(X_t)
        return m[:, cols], np.abs(v[:, cols])

    def predictive(self, Xpred, route="default"):
        """svmogp.py:333-351: predictive mean / variance of every output at Xpred[t].

        route="default"    q(f_d)(Xpred) straight from q(u) -- `calculate_q_f` at the new inputs, i.e. the reference's OWN
                           `predictive_new` semantics (svmogp.py:280-306) -- on the device, any N.  NOT what the reference's
                           `predictive` returns: that one goes through `_raw_predict_f`.
        route="reference"  the reference's route: `_raw_predict_f` per function (O(N^3) in the training rows of the task,
                           limited to REFERENCE_ROUTE_MAX_ROWS), then `<likelihood>.predictive` with the Gauss-Hermite rule
                           a trained reference model reads (Gamma / Beta: the cached 10-point rule, GPy `_gh_points` quirk)."""
        m_F, v_F = [], []
        for t in range(len(self.likelihood.likelihoods_list)):
            m, v = self._predict_route(Xpred[t], t, route)
            m_F.append(m)
            v_F.append(v)
        if route == "reference":
            from .engine import predictive as lik_predictive
            out = [lik_predictive(l.name, m_F[t], v_F[t], gh_T=10 if l.name in ("Gamma", "Beta") else 0,
                                  device=self._engine_device(), **l.kwargs())
                   for t, l in enumerate(self.likelihood.likelihoods_list)]
            return [o[0] for o in out], [o[1] for o in out]
        return self.likelihood.predictive(m_F, v_F, self.Y_metadata)

    def natural_gradient_step(self, gamma=1.0):
        """q(u) <- natural-gradient step of size gamma (not in the reference; named in the north-star).  Uses the
        gradients of the last `parameters_changed()`; updates q_u_means / q_u_chols and re-evaluates."""
        self._refresh()
        m, L = self._engine.natgrad_step(gamma)
        self.q_u_means[...] = m
        self.q_u_chols[...] = L
        self.parameters_changed()
        return self

    def log_predictive_density(self, Xtest, Ytest, route="default", gh_T=0, return_ess=False):
        """Deterministic held-out score: per task an (N_t,) array of per-row log predictive densities, the log of the
        Gauss-Hermite rule of p(y | f) under q(f) at the test inputs.  Defined for every likelihood (Gamma and Beta included), no
        seed, no sampling noise.  route="default": q(f) is formed on the device and feeds the rule there with the engine's current
        likelihood parameters (`hmogp_predict_log_density`); route="reference": q(f) from `_raw_predict_f`, then the stand-alone
        building block with the likelihoods' current kwargs.  return_ess=True: (lpd list, ess list).  One RuntimeWarning per call
        when some row's effective number of nodes is below its family's `likelihoods.LPD_ESS_WARN` (the rule cannot resolve such a row)."""
        from .engine import log_predictive_density_rows
        from .likelihoods import warn_low_ess
        if route not in ("default", "reference"):
            raise ValueError("route must be 'default' or 'reference'")
        lpd, ess = [], []
        for t, l in enumerate(self.likelihood.likelihoods_list):
            if route == "default":
                self._refresh()
                a, e = self._engine.predict_log_density(t, np.asarray(Xtest[t], dtype=float).reshape(-1, self.Xdim), Ytest[t], gh_T=gh_T)
            else:
                m, v = self._predict_route(Xtest[t], t, route)
                a, e = log_predictive_density_rows(l.name, Ytest[t], m, v, gh_T=gh_T, return_ess=True, device=self._engine_device(),
                                                   **l.kwargs())
            lpd.append(a)
            ess.append(e)
        warn_low_ess(ess, self.likelihood.specs())
        return (lpd, ess) if return_ess else lpd

    def _predq_tasks(self, tasks, route):
        if route not in ("default", "reference"):
            raise ValueError("route must be 'default' or 'reference'")
        return self.likelihood._predq_tasks(tasks)           # (NotImplementedError before anything is launched)

    def predict_quantiles(self, Xpred, quantiles=(2.5, 97.5), tasks=None, route="default", gh_T=0):
        """Predictive quantiles of the outputs at Xpred[t] (GPy's `predict_quantiles`): `quantiles` are PERCENTAGES, the
        result one (N_t, len(quantiles)) array per requested task, in the order of `tasks` (None: all tasks).  Built for Gaussian,
        HetGaussian, Bernoulli, Exponential, Ordinal and Weibull; any other family among the requested tasks raises NotImplementedError
        naming it and the special function its cdf needs.  route="default": q(f) on the device, the engine's current likelihood
        parameters (`hmogp_predict_quantile`); route="reference": q(f) from `_raw_predict_f`, then the stand-alone building block."""
        from .engine import predictive_quantile_rows
        probs = np.asarray(quantiles, dtype=float).reshape(-1) / 100.0
        out = []
        for t in self._predq_tasks(tasks, route):
            l = self.likelihood.likelihoods_list[t]
            if route == "default":
                self._refresh()
                out.append(self._engine.predict_quantile(t, np.asarray(Xpred[t], dtype=float).reshape(-1, self.Xdim), probs, gh_T=gh_T))
            else:
                m, v = self._predict_route(Xpred[t], t, route)
                out.append(predictive_quantile_rows(l.name, m, v, probs, gh_T=gh_T, device=self._engine_device(), **l.kwargs()))
        return out

    def predictive_cdf(self, Xtest, Ytest, return_sf=False, tasks=None, route="default", gh_T=0):
        """Predictive cdf P(Y <= y) of the rows (Xtest[t], Ytest[t]): one (N_t,) array per requested task, or a (cdf, sf)
        pair with return_sf=True -- sf = P(Y > y) summed on its own, never 1 - cdf.  Xtest / Ytest are indexed by task; Ytest[t] is
        (N_t,): values, Ordinal labels, Weibull times.  Families, tasks and routes as in `predict_quantiles`."""
        from .engine import predictive_cdf_rows
        out = []
        for t in self._predq_tasks(tasks, route):
            l = self.likelihood.likelihoods_list[t]
            if route == "default":
                self._refresh()
                c, s_ = self._engine.predict_cdf(t, np.asarray(Xtest[t], dtype=float).reshape(-1, self.Xdim), Ytest[t], gh_T=gh_T)
            else:
                m, v = self._predict_route(Xtest[t], t, route)
                c, s_ = predictive_cdf_rows(l.name, Ytest[t], m, v, gh_T=gh_T, return_sf=True, device=self._engine_device(), **l.kwargs())
            out.append((c, s_) if return_sf else c)
        return out

    def survival_function(self, t, X, times, gh_T=0):
        """Survival curves S(time | x) of the Weibull task t: (N, len(times)), row n the probability that the event at
        X[n] is later than each of `times`.  q(f) is formed once with `predict_f`; the building block then runs on the tiled rows."""
        from .engine import predictive_cdf_rows
        l = self.likelihood.likelihoods_list[int(t)]
        if l.name != "Weibull":
            raise ValueError("survival_function: task %d is %s, not Weibull" % (int(t), l.name))
        times = np.asarray(times, dtype=float).reshape(-1)
        m, v = self._predict_route(np.asarray(X, dtype=float).reshape(-1, self.Xdim), int(t), "default")
        n, k = m.shape[0], times.shape[0]
        _, sf = predictive_cdf_rows("Weibull", np.tile(times, n), np.repeat(m, k, axis=0), np.repeat(v, k, axis=0), gh_T=gh_T,
                                    return_sf=True, device=self._engine_device())
        return sf.reshape(n, k)

    def negative_log_predictive(self, Xtest, Ytest, num_samples=1000, seed=0, route="default", method="mc"):
        """svmogp.py:353-370.  q(f) at the test inputs: route="default" from `predict_f`, route="reference" through
        `_raw_predict_f` as the reference does (see `predictive`).  method="mc" (default): the reference's Monte-Carlo estimate with
        its 1/num_samples factor; method="quadrature": minus the sum of all rows of `log_predictive_density` -- deterministic, defined
        for every likelihood, without that factor; num_samples and seed are ignored."""
        if method == "quadrature":
            return -float(sum(np.sum(a) for a in self.log_predictive_density(Xtest, Ytest, route=route)))
        if method != "mc":
            raise ValueError("method must be 'mc' or 'quadrature'")
        mu, vv = [], []
        for t in range(len(self.Ymulti_all)):
            m, v = self._predict_route(Xtest[t], t, route)
            mu.append(m)
            vv.append(v)
        return self.likelihood.negative_log_predictive(Ytest, mu, vv, Y_metadata=self.Y_metadata, num_samples=num_samples,
                                                       seed=seed)

    def timings(self):
        return self._engine.timings()


HetMOGP = SVMOGP  # the README's name for the class (README.md:35); the reference's code only defines SVMOGP


class PosteriorPaths(object):
    """`size` posterior sample paths of a model's functions as functions (`SVMOGP.sample_paths`; pathwise conditioning).
    `paths(Xnew)` -> (size, N, nD), the orientation of `posterior_samples_f`: the same draw on every call, at any inputs.  A snapshot
    of the model at the time of the draw.  A context manager; `close()` frees the set on the device, any use after it raises."""

    def __init__(self, model, size, functions, num_features, seed):
        self._engine = model._engine
        self._xdim = model.Xdim
        self.functions = list(range(model.num_output_funcs)) if functions is None else [int(f) for f in np.ravel(functions)]
        self.size, self.num_features, self.seed = int(size), int(num_features), int(seed)
        self._id = None
        self._id = self._engine.paths_create(functions, size=self.size, num_features=self.num_features, seed=self.seed)

    def _live(self):
        if self._id is None:
            raise ValueError("PosteriorPaths: the path set is closed")
        return self._id

    def __call__(self, Xnew):
        F = self._engine.paths_eval(self._live(), np.asarray(Xnew, dtype=float).reshape(-1, self._xdim))
        return np.ascontiguousarray(np.transpose(F, (0, 2, 1)))

    def grad(self, Xnew):
        """The gradients of the paths with respect to the inputs: (size, N, nD, P), [s, i, j, p] = d f_j^s / d x_p at row i -- the
        exact derivative of the function `paths(Xnew)` evaluates, for gradient ascent on a sample path."""
        G = self._engine.paths_eval_grad(self._live(), np.asarray(Xnew, dtype=float).reshape(-1, self._xdim))
        return np.ascontiguousarray(np.transpose(G, (0, 2, 1, 3)))

    def value_and_grad(self, Xnew):
        """(`paths(Xnew)` (size, N, nD), `grad(Xnew)` (size, N, nD, P)) from one pass over Xnew; the values are the bits of `paths(Xnew)`."""
        F, G = self._engine.paths_eval_grad(self._live(), np.asarray(Xnew, dtype=float).reshape(-1, self._xdim), values=True)
        return np.ascontiguousarray(np.transpose(F, (0, 2, 1))), np.ascontiguousarray(np.transpose(G, (0, 2, 1, 3)))

    def state(self):
        """dict(omega (Q, Lf, P), theta (Q, 2 Lf, size, nD), v (Q, M, size, nD), u (Q, size, M)): the set's frequencies and weights."""
        return self._engine.paths_state(self._live())

    def close(self):
        sid, self._id = self._id, None
        if sid is not None and getattr(self._engine, "_h", None):
            self._engine.paths_free(sid)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
