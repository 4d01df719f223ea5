"""DGPSSM: the model object whose `nll` is the hot path -- counterpart of vfegpssm/dgp_model.py:160-324.

The reference builds a TensorFlow graph whose root tensor is `self.nll` and evaluates it with
`session.run` (base_model.py:952-989).  Here the same quantities are methods backed by one ElboEngine
(hand-written HIP kernels behind the C ABI); parameters live in NumPy arrays on the object with the
reference's attribute names (layers[-1].X / .U / .Z, kernels, log_Q, likelihood.CC / .DD / .log_Rchols).
"""
from __future__ import annotations

import copy

import numpy as np

from .engine import ElboEngine
from .kernels import stack_hypers


class Layer:
    """Layer.__init__ (dgp_model.py:46-94): variables X (T+1, D), U (M, D), Z (M, P) and the kernel list."""

    def __init__(self, ZZ, U_ini, X_0_ini, X_train_ini, kern, outputs, n_inducing, x_dims_l, Y_len,
                 prior_type="uniform", kernel_type="SquaredExponential"):
        self.inputs, self.outputs, self.kernel, self.kernel_type = kern[0].input_dim, outputs, kern, kernel_type
        self.M = n_inducing
        self.prior_type = prior_type
        X_ini_val = np.zeros((Y_len + 1, x_dims_l))            # dgp_model.py:56
        X_ini_val[0] = X_0_ini                                 # :57
        X_ini_val[1:] = X_train_ini                            # :58
        self.X = X_ini_val
        self.U = np.array(U_ini, dtype=np.float64)             # :66
        self.Z = np.array(ZZ, dtype=np.float64)                # :67


class DGPSSM:
    """One-layer GP state-space model; `nll()` / `nll_terms()` evaluate dgp_model.py:248-297 on the GPU.

    Constructor arguments keep the reference's names (dgp_model.py:160-166).  `num_chains` > 1 evaluates
    S latent trajectories X_s in one call (`set_X`), which is what BASELINE.json's metric measures."""

    ROLLOUT_MODES = ("reference", "intent", "intent-batched", "intent-fused")      # collect_samples_formal(rollout_mode=...)

    def __init__(self, Y, x_dims, n_inducing, kernels, likelihood, minibatch_size=None, window_size=64,
                 output_dim=None, prior_type="uniform", full_cov=False, epsilon=0.01, mdecay=0.05, QQ_chol=None,
                 ZZ=None, variance=None, lengthscales=None, control_inputs=None, kernel_type="SquaredExponential",
                 kernel_train_flag=True, U_ini=None, X_0_ini=None, X_train_ini=None, X_PG=False, PG_particles=100,
                 hyperparameter_sampling=False, kernel_optimization=False, U_optimization=False, U_collapse=False,
                 Z_optimization=False, case_val=1, num_chains=1, device=0, **engine_kw):
        if full_cov:
            raise NotImplementedError("full_cov=True is not used by the GP-SSM path (FFVD_Main.py:266)")
        if len(kernels) != 1:
            raise NotImplementedError("n_layers != 1 (FFVD_Main.py:360 default 1; the nll uses layers[-1] only)")
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]                                      # models.py:44-45
        self.Y = Y
        self.x_dims, self.n_inducing, self.kernels, self.likelihood = x_dims, n_inducing, kernels, likelihood
        self.minibatch_size, self.window_size = minibatch_size, window_size
        self.output_dim = output_dim or x_dims[-1]
        self.kernel_type, self.U_collapse, self.case_val = kernel_type, bool(U_collapse), case_val
        self.prior_type = prior_type
        self.log_Q = np.array(2.0 * np.log(np.asarray(QQ_chol, dtype=np.float64)))     # dgp_model.py:182
        kern = kernels[-1]
        D = self.output_dim
        if len(kern) != D:
            raise ValueError(f"expected one kernel per latent dim ({D}), got {len(kern)}")
        self.layers = [Layer(ZZ, U_ini, X_0_ini, X_train_ini, kern, D, n_inducing, x_dims[-1], Y.shape[0],
                             prior_type=prior_type, kernel_type=kernel_type)]
        self.X_N = self.layers[-1].X.shape[0]
        T = self.X_N - 1
        if control_inputs is None or np.asarray(control_inputs).shape[0] == 0:
            self.control_inputs = np.zeros((T, 0))
        else:
            self.control_inputs = np.asarray(control_inputs, dtype=np.float64)
        C = self.control_inputs.shape[1]
        self.num_chains = int(num_chains)
        self._X_chains = np.repeat(self.layers[-1].X[None], self.num_chains, axis=0)
        self.engine = ElboEngine(T, D, C, n_inducing, self.num_chains, Ydim=Y.shape[1], kernel_type=kernel_type,
                                 U_collapse=self.U_collapse, prior_type=prior_type, device=device, **engine_kw)
        self.engine.set_data(Y, self.control_inputs)
        self._last = None
        self.epsilon, self.mdecay = epsilon, mdecay
        self.X_PG, self.PG_particles = bool(X_PG), int(PG_particles)
        self.PG_mode = "intent"        # "reference" reproduces the reference's no-op (see gp_x_sampling)
        # which variables SG-HMC samples and which Adam trains (dgp_model.py:213-244):
        # case 4 (collapsed U, kernel/Z optimisation on: what FFVD_Main.py:300-305 sets) leaves `vars` empty
        self.vars = []
        if not kernel_optimization and kernel_train_flag:                       # :224-232
            self.vars += ["logvariance", "loglengthscales"] if kernel_type == "SquaredExponential" else ["logvariance"]
        if not U_optimization and not self.U_collapse:                           # :234-236
            self.vars += ["U"]
        if not Z_optimization:                                                   # :240-242
            self.vars += ["Z"]
        if hyperparameter_sampling:                                              # :244-246
            self.vars += ["log_Q", "CC", "DD", "log_Rchols"]
        # what AdamOptimizer.minimize(nll) (dgp_model.py:303-305) updates = the variables created with trainable=True:
        # X unless X_PG or case 7 (:62-66); U iff U_optimization (:68), Z iff Z_optimization (:69); the kernel
        # hyper-parameters iff kernel_optimization (kernels_multi_output.py:156,160); log_Q unless hyperparameter_sampling
        # or case 7 (:176-184); CC, DD, log_Rchols iff likelihood_traning and not hyperparameter_sampling
        # (likelihoods.py:14-24,47-55).  A variable that is neither trainable nor in `vars` simply stays put.
        train = []
        if not (self.X_PG or case_val == 7):
            train.append("X")
        if Z_optimization:
            train.append("Z")
        if kernel_optimization:
            train += ["logvariance", "loglengthscales"]
        if not hyperparameter_sampling and case_val != 7:
            train.append("log_Q")
        if getattr(likelihood, "trainable", True):
            train += ["CC", "DD", "log_Rchols"]
        if U_optimization and not self.U_collapse:
            train.append("U")
        self._adam_train = tuple(k for k in train if k not in self.vars)
        self._rng = np.random.default_rng()
        self.window = []
        self._resident = False      # device copy of the parameters is current (set by train_hypers)
        self._host_stale = False    # ... and newer than the NumPy attributes

    @property
    def Q(self):
        return np.exp(self.log_Q)                               # dgp_model.py:186

    def set_X(self, X_chains):
        """Latent trajectories to evaluate: (S, T+1, D) (or (T+1, D) for one chain)."""
        if self._host_stale:
            self.pull_parameters()
        self._resident = False
        X = np.asarray(X_chains, dtype=np.float64)
        if X.ndim == 2:
            X = X[None]
        if X.shape != self._X_chains.shape:
            raise ValueError(f"X: expected {self._X_chains.shape}, got {X.shape}")
        self._X_chains = X
        self.layers[-1].X = X[0]

    def parameters(self):
        """The parameter dictionary the engine consumes, gathered from the reference-named attributes."""
        lay = self.layers[-1]
        _, _, logvar, loglen = stack_hypers(lay.kernel)
        return dict(X=self._X_chains, Z=lay.Z, U=lay.U, logvariance=logvar, loglengthscales=loglen,
                    log_Q=self.log_Q, CC=self.likelihood.CC, DD=self.likelihood.DD,
                    log_Rchols=self.likelihood.log_Rchols)

    def nll_terms(self):
        """nll and the named component tensors of dgp_model.py:264-297 (mean over chains)."""
        self._last = self.engine.nll_terms(None if self._resident else self.parameters())
        return self._last

    def nll(self):
        return self.nll_terms()["nll"]

    def print_sample_performance(self):
        """Counterpart of BaseModel.print_sample_performance (base_model.py:952-989): the component breakdown."""
        t = self.nll_terms()
        for k, v in t.items():
            if k != "nll_per_chain":
                print(f"{k}: {v}")
        return t

    # ---- training loop pieces (models.py:142-182 drives these) -----------------------------------------
    def get_minibatch(self, global_step=1):
        """BaseModel.get_minibatch (base_model.py:188-194): full batch, lr = 0.003 * 0.95^(global_step/1000)."""
        return [0, self.X_N], 0.003 * (0.95 ** (global_step / 1000))

    def nll_and_grad(self):
        """nll terms + d nll / d variables (what tf.gradients(nll, vars), base_model.py:148, hands the optimisers)."""
        return self.engine.nll_and_grad(None if self._resident else self.parameters())

    def seed(self, seed):
        """Seed the generator behind the SG-HMC noise draws and the window choice of train_hypers (the reference
        draws both unseeded, base_model.py:169,948)."""
        self._rng = np.random.default_rng(seed)

    def _noise(self):
        shapes = {"Z": self.layers[-1].Z.shape, "logvariance": (self.output_dim,),
                  "loglengthscales": (self.output_dim, self.engine.P), "log_Q": (self.output_dim,),
                  "CC": self.likelihood.CC.shape, "DD": self.likelihood.DD.shape,
                  "log_Rchols": self.likelihood.log_Rchols.shape, "U": self.layers[-1].U.shape}
        return {k: self._rng.standard_normal(shapes[k]) for k in self.vars}

    def _ensure_resident(self):
        if not self._resident:
            self.engine.set_params(self.parameters())
            self._resident = True

    def sghmc_step(self):
        """BaseModel.sghmc_step (base_model.py:915-933): burn_in_op, then 10 x (burn_in_op, sample_op) on
        `self.vars` -- each one forward + backward + SG-HMC update on the device -- and the current values of the
        variables join the window.  With an empty variable list (cases 1, 4, 6) the ops are no-ops; cases 2 and 3 sample
        the kernel hyper-parameters, U (and Z), case 5 the kernel hyper-parameters."""
        if not self.vars:
            self.window.append({})
        else:
            self._ensure_resident()
            self.engine.sghmc_step(self._noise(), self.epsilon, self.mdecay, burn_in=True)            # :919
            for _ in range(10):                                                                       # :920-925
                self.engine.sghmc_step(self._noise(), self.epsilon, self.mdecay, burn_in=True)
                self.engine.sghmc_step(self._noise(), self.epsilon, self.mdecay, burn_in=False)
            self._host_stale = True
            g = self.engine.get_params()
            self.window.append({k: g[k].copy() for k in self.vars})                                   # :927-930
        if len(self.window) > self.window_size:
            self.window = self.window[-self.window_size:]                                             # :931-933

    def train_hypers(self):
        """BaseModel.train_hypers (base_model.py:944-950): one Adam step on nll w.r.t. every variable that SG-HMC
        does not sample, with the sampled ones fed from a random window entry for this step only (:948-949);
        forward + backward + update on the device.  Returns the nll terms before the update."""
        self._ensure_resident()
        _, lr = self.get_minibatch()
        fed = self.window[int(self._rng.integers(len(self.window)))] if (self.vars and self.window) else {}
        if fed:
            cur = self.engine.get_params()
            self.engine.update_params(fed)
        t = self.engine.adam_step(lr, train=self._adam_train)
        if fed:
            self.engine.update_params({k: cur[k] for k in fed})        # feed_dict does not assign: restore the chain state
        self._host_stale = True
        return t

    def gp_x_sampling(self, mode=None):
        """`gp_x_sampling()` of the training loop (models.py:156-158) = `pg_x_sampling_op = PG_for_X_speedup(...)`
        (dgp_model.py:309, base_model.py:78-138).

        mode "reference": exactly what the reference's op does -- nothing: its TensorArray writes are discarded (:115)
        and the final assign is never run (:137), X stays as it is.
        mode "intent" (default): one particle-Gibbs sweep per chain on the device (`ffvd_op_pg_sweep`):
        PG_particles - 1 free particles from N(0, I) (:79) advanced with the explicit-U conditional (:93-101),
        weighted against Y (:105-109), resampled together with the current trajectory as the conditioned particle
        (:111-115); a uniformly drawn slot replaces X unless it is the conditioned one (:135-137).
        Returns the number of chains whose trajectory was replaced."""
        mode = mode or self.PG_mode
        if mode == "reference":
            return 0
        if mode != "intent":
            raise ValueError("PG mode must be 'reference' or 'intent'")
        if self.U_collapse:
            raise ValueError("PG_for_X_speedup conditions on the explicit U (base_model.py:96): U_collapse must be False")
        from . import conditionals_multi_output as cmo
        from .prediction import pg_sweep
        if self._host_stale:
            self.pull_parameters()
        lay = self.layers[-1]
        n1 = self.PG_particles - 1
        if n1 < 1:
            raise ValueError("PG_particles must be at least 2")
        T, D = self.X_N - 1, self.output_dim
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)                                             # :81
        Rch = np.exp(np.asarray(self.likelihood.log_Rchols, dtype=np.float64))                  # likelihood.Rchols
        Rch = np.tril(Rch) if Rch.shape[0] > 1 else Rch
        Q = np.exp(self.log_Q)
        replaced = 0
        Xc = np.array(self._X_chains, dtype=np.float64, copy=True)
        for s_ in range(self.num_chains):
            x0 = self._rng.standard_normal((n1, D))                                           # :79
            eps = self._rng.standard_normal((T, n1, D))                                       # :101
            unif = self._rng.random((T, n1))                                                  # :113
            parts, _ = pg_sweep(Lm, lay.Z, lay.kernel, lay.U, Xc[s_], self.Y, self.control_inputs, self.likelihood.CC,
                                self.likelihood.DD, Rch, Q, x0, eps, unif)
            final_index = int(self._rng.integers(self.PG_particles))                          # :135
            if final_index < n1:                                                              # :136-137
                Xc[s_] = parts[:, final_index]
                replaced += 1
        if replaced:
            self._X_chains = Xc
            lay.X = Xc[0]
            if self._resident:
                self.engine.update_params({"X": Xc})
        return replaced

    def pull_parameters(self):
        """Copy the trained parameters from the device back into the reference-named attributes."""
        g = self.engine.get_params()
        lay = self.layers[-1]
        self._X_chains = g["X"]
        lay.X, lay.Z = g["X"][0], g["Z"]
        if not self.U_collapse:
            lay.U = g["U"]
        for d, k in enumerate(lay.kernel):
            k.logvariance = np.float64(g["logvariance"][d])
            if hasattr(k, "loglengthscales"):
                k.loglengthscales = g["loglengthscales"][d].copy()
        self.log_Q = g["log_Q"]
        self.likelihood.CC, self.likelihood.DD, self.likelihood.log_Rchols = g["CC"], g["DD"], g["log_Rchols"]
        self._host_stale = False
        return g

    def sample_op(self, noise=None):
        """One `sample_op` of generate_update_step (base_model.py:171-179) on `self.vars`: forward + backward + SG-HMC
        update of theta and p on the device.  `noise`: name -> standard-normal array (default: the model's generator)."""
        self._ensure_resident()
        t = self.engine.sghmc_step(self._noise() if noise is None else noise, self.epsilon, self.mdecay, burn_in=False)
        self._host_stale = True
        return t

    def collect_samples_formal(self, num, spacing, control_inputs, test_len, sghmc_var_len=0, U_collapse=None,
                               Y_test=None, Y_train_std=1.0, save_path_file=None, Y_train=None, case="C1", ll_seq=(0.0,),
                               running_time_seq=(0.0,), PG_num=None, synthetic_data_function_plot=False, data_uu=None,
                               eps=None, seed=None, rollout_mode="reference"):
        """BaseModel.collect_samples_formal (base_model.py:197-517), called as FFVD_Main.py:345-349 does: K_uu factors,
        posterior U (collapsed branch), `num` rollouts of `test_len` steps from X[-1], predictive y mean / variance, the
        RMSE over the first 30 test points and, with `save_path_file`, the `_results.npz` of :512-517.

        sghmc_var_len > 0 (cases 2, 3, 5: `len(model.vars)`): before rollout num_i the reference runs `spacing` x
        `sample_op` (:223-231) and records the variables (:239-240).  rollout_mode:
          "reference" -- what the reference's graph computes: its rollout tensors are only EVALUATED by the one
                         session.run at :326-327, after the last sample_op, so every rollout sees the final variable
                         values; the `num` rollouts differ by their noise only;
          "intent"    -- rollout num_i uses the variables as they are after its own sample_ops (K_uu factors and
                         posterior U recomputed per sample), which is what the loop sets out to do;
          "intent-batched" -- the same sampler sequence and the same per-sample posteriors as "intent", with the `num` rollouts
                         deferred into ONE `rollout_grouped` call (G = num posteriors, R = 1) after the last sample_op;
          "intent-fused" -- the sampler sequence and the recorded variables of "intent-batched"; per sample only Z, the kernels,
                         chain 0's X and Q are kept, and after the last sample_op ONE `posterior_rollout_grouped` call (G = num,
                         R = 1, one model per group) forms the `num` posteriors and their rollouts without the posteriors leaving
                         the device.  Collapsed branch only: with explicit U it is "intent-batched".
        `eps` (test_len, num, D) injects the standard-normal draws of :306 (else numpy's default_rng(seed)); the
        SG-HMC noise comes from the model's generator (`seed()`).  Returns a dict and sets the reference's attributes
        (fit_x, predict_y, predict_y_var, fit_y, RMSE_val)."""
        from . import conditionals_multi_output as cmo
        from .prediction import posterior_rollout_grouped, predict_y_summary, rollout, rollout_grouped
        if synthetic_data_function_plot:
            raise NotImplementedError("synthetic_data_function_plot: plotting aid of the kink toy problem, not on the GP-SSM path")
        if rollout_mode not in self.ROLLOUT_MODES:
            raise ValueError("rollout_mode must be 'reference', 'intent', 'intent-batched' or 'intent-fused'")
        if sghmc_var_len and sghmc_var_len != len(self.vars):
            raise ValueError(f"sghmc_var_len = {sghmc_var_len} but the model samples {len(self.vars)} variables")
        if self._host_stale:
            self.pull_parameters()
        U_collapse = self.U_collapse if U_collapse is None else bool(U_collapse)
        D = self.output_dim
        ci = self.control_inputs if control_inputs is None else np.asarray(control_inputs, dtype=np.float64)
        T = self.X_N - 1
        self.fit_x = self.layers[-1].X.copy()                                                  # :203
        if eps is None:
            eps = np.random.default_rng(seed).standard_normal((test_len, num, D))
        eps = np.asarray(eps, dtype=np.float64)
        n_train = self.Y.shape[0] if Y_train is None else np.asarray(Y_train).shape[0]

        def posterior():
            lay = self.layers[-1]
            Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)                                          # :207 / :234
            if U_collapse:
                xc = np.concatenate((lay.X[:T], ci[:T]), axis=1) if ci.shape[1] > 0 else lay.X[:-1]    # :243-246
                U_val, U_chol = cmo.collapse_u_mean_after_kernel_precalculation(Lm, xc, lay.X, lay.Z, lay.kernel, self.Q)  # :251
            else:
                U_val, U_chol = lay.U, None                                                     # :255-256
            return Lm, U_val, U_chol

        mc = [[] for _ in self.vars]
        px_parts, pv_parts = [], []
        groups = []                                                                             # "intent-batched": one posterior per sample
        fused_groups = []                                                                       # "intent-fused": one model per sample
        if sghmc_var_len:
            for num_i in range(num):
                for _ in range(spacing):                                                        # :225-231
                    self.sample_op()
                self.pull_parameters()
                cur = self.parameters()
                for i, k in enumerate(self.vars):
                    mc[i].append(np.array(cur[k], copy=True))                                   # :239-240
                if rollout_mode == "intent":
                    Lm, U_val, U_chol = posterior()
                    lay = self.layers[-1]
                    px, pv = rollout(Lm, lay.Z, lay.kernel, U_val, U_chol, lay.X[-1], ci, n_train, test_len, self.Q,
                                     eps[:, num_i:num_i + 1])
                    px_parts.append(px)
                    pv_parts.append(pv)
                elif rollout_mode == "intent-fused" and U_collapse:
                    lay = self.layers[-1]
                    fused_groups.append((np.array(lay.Z, copy=True), copy.deepcopy(lay.kernel), np.array(lay.X, copy=True),
                                         np.array(self.Q, copy=True)))
                elif rollout_mode in ("intent-batched", "intent-fused"):
                    Lm, U_val, U_chol = posterior()
                    lay = self.layers[-1]
                    groups.append((Lm, np.array(lay.Z, copy=True), copy.deepcopy(lay.kernel), U_val, U_chol,
                                   np.array(lay.X[-1], copy=True), np.array(self.Q, copy=True)))
        if groups:
            cols = list(zip(*groups))
            px, pv = rollout_grouped(cols[0], cols[1], cols[2], cols[3], cols[4] if U_collapse else None, cols[5], ci, n_train,
                                     test_len, cols[6], eps[:, :, None, :])
            px, pv = px[:, 0], pv[:, 0]
            U_val = U_val if U_collapse else self.layers[-1].U
        elif fused_groups:
            cols = list(zip(*fused_groups))
            px, pv, U_all = posterior_rollout_grouped(cols[0], cols[1], cols[2], cols[3], ci, n_train, test_len, eps[:, :, None, :],
                                                      return_U=True)
            px, pv, U_val = px[:, 0], pv[:, 0], U_all[-1]
        elif px_parts:
            px, pv = np.concatenate(px_parts, axis=0), np.concatenate(pv_parts, axis=0)
            U_val = U_val if U_collapse else self.layers[-1].U
        else:
            Lm, U_val, U_chol = posterior()
            lay = self.layers[-1]
            px, pv = rollout(Lm, lay.Z, lay.kernel, U_val, U_chol, lay.X[-1], ci, n_train, test_len, self.Q, eps)
        lay = self.layers[-1]
        out = predict_y_summary(px, pv, self.likelihood.CC, self.likelihood.DD, self.likelihood.log_Rchols, Y_test,
                                Y_train_std)
        self.predict_y, self.predict_y_var = out["predict_y"], out["predict_y_var"]
        self.fit_y = (np.asarray(self.fit_x)[1:] @ self.likelihood.CC + self.likelihood.DD).reshape(-1)   # :344
        if "RMSE" in out:
            self.RMSE_val = out["RMSE"]
            print("RMSE: ", self.RMSE_val)                                                      # :350
        out.update(predict_x=px, predict_x_var=pv, U_val=U_val, fit_y=self.fit_y,
                   mc_posterior_samples={k: np.stack(v) for k, v in zip(self.vars, mc) if v})
        if save_path_file is not None:                                                         # :486-517
            from .data_io import save_results
            out["results_file"] = save_results(save_path_file, self, Y_test, Y_train, Y_train_std, case=case, ll_seq=ll_seq,
                                               running_time_seq=running_time_seq, PG_num=PG_num,
                                               mc_posterior_samples=out["mc_posterior_samples"])
        return out

    def collect_samples_chains(self, num_per_chain, control_inputs, test_len, *, Y_test=None, Y_train_std=1.0, Y_train=None,
                               eps=None, seed=None, fused=False, summary="host"):
        """Rollouts from EVERY chain of a `num_chains = S` model (collect_samples_formal predicts from chain 0 only): the K_uu
        factors once, the collapsed posterior U | X_s per chain (with explicit U: the shared U, no q_sqrt), `num_per_chain`
        rollouts of `test_len` steps from each chain's own X_s[-1] -- one `rollout_grouped` call with G = S, R = num_per_chain.
        `eps` (test_len, S, num_per_chain, D) injects the draws of base_model.py:306 (else numpy's default_rng(seed)).
        fused=True (collapsed U only; ValueError with explicit U: there is no posterior to build): the S posteriors and their rollouts
        in ONE `posterior_rollout_grouped` call with the model shared by the groups -- the posteriors never leave the device.
        summary "host": `predict_y_summary` in NumPy on the downloaded stacks; "device": the same keys from the summary kernels in
        the same call (`rollout_grouped_summary` / `posterior_rollout_grouped_summary`), plus predict_y_var_total and, with Y_test,
        lpd, lpd_gauss, ll and ll_original_units (prediction.rollout_summary).
        Returns a dict: predict_x, predict_x_var (S, num_per_chain, test_len, D) and the predict_y_summary over all S * R rollouts."""
        from . import conditionals_multi_output as cmo
        from .prediction import (posterior_rollout_grouped, posterior_rollout_grouped_summary, predict_y_summary, rollout_grouped,
                                 rollout_grouped_summary)
        if summary not in ("host", "device"):
            raise ValueError("collect_samples_chains: summary must be 'host' or 'device'")
        if fused and not self.U_collapse:
            raise ValueError("collect_samples_chains: fused=True builds the collapsed posterior; with explicit U there is none to build")
        if self._host_stale:
            self.pull_parameters()
        S, D, T, R = self.num_chains, self.output_dim, self.X_N - 1, int(num_per_chain)
        if R < 1:
            raise ValueError("num_per_chain must be at least 1")
        ci = self.control_inputs if control_inputs is None else np.asarray(control_inputs, dtype=np.float64)
        if eps is None:
            eps = np.random.default_rng(seed).standard_normal((test_len, S, R, D))
        eps = np.asarray(eps, dtype=np.float64)
        if eps.shape != (test_len, S, R, D):
            raise ValueError(f"eps: expected {(test_len, S, R, D)}, got {eps.shape}")
        n_train = self.Y.shape[0] if Y_train is None else np.asarray(Y_train).shape[0]
        lay = self.layers[-1]
        lik = self.likelihood
        if fused and summary == "device":
            out = posterior_rollout_grouped_summary(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train,
                                                    test_len, eps, lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std,
                                                    return_rollouts=True, return_U=True)
            U_all = out.pop("U_means")
            out["U_vals"] = [U_all[s_] for s_ in range(S)]
            return out
        if fused:
            px, pv, U_all = posterior_rollout_grouped(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train,
                                                      test_len, eps, return_U=True)
            out = predict_y_summary(px.reshape(S * R, test_len, D), pv.reshape(S * R, test_len, D), self.likelihood.CC,
                                    self.likelihood.DD, self.likelihood.log_Rchols, Y_test, Y_train_std)
            out.update(predict_x=px, predict_x_var=pv, U_vals=[U_all[s_] for s_ in range(S)])
            return out
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        U_vals, U_chols = [], []
        for s_ in range(S):
            Xs = self._X_chains[s_]
            if self.U_collapse:
                xc = np.concatenate((Xs[:T], ci[:T]), axis=1) if ci.shape[1] > 0 else Xs[:-1]
                U_val, U_chol = cmo.collapse_u_mean_after_kernel_precalculation(Lm, xc, Xs, lay.Z, lay.kernel, self.Q)
            else:
                U_val, U_chol = lay.U, None
            U_vals.append(U_val)
            U_chols.append(U_chol)
        if summary == "device":
            out = rollout_grouped_summary([Lm] * S, [lay.Z] * S, [lay.kernel] * S, U_vals, U_chols if self.U_collapse else None,
                                          [self._X_chains[s_][-1] for s_ in range(S)], ci, n_train, test_len, [self.Q] * S, eps,
                                          lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std, return_rollouts=True)
            out["U_vals"] = U_vals
            return out
        px, pv = rollout_grouped([Lm] * S, [lay.Z] * S, [lay.kernel] * S, U_vals, U_chols if self.U_collapse else None,
                                 [self._X_chains[s_][-1] for s_ in range(S)], ci, n_train, test_len, [self.Q] * S, eps)
        out = predict_y_summary(px.reshape(S * R, test_len, D), pv.reshape(S * R, test_len, D), self.likelihood.CC,
                                self.likelihood.DD, self.likelihood.log_Rchols, Y_test, Y_train_std)
        out.update(predict_x=px, predict_x_var=pv, U_vals=U_vals)
        return out

    def evaluate_heldout(self, Y_test, control_inputs, num_per_chain, *, Y_train_std=1.0, eps=None, seed=None, method="rollouts"):
        """Held-out metrics of the model as it stands: `num_per_chain` rollouts of len(Y_test) steps from every chain's X_s[-1],
        summarised on the device (prediction.rollout_summary has the quantities) -- no trajectory is downloaded.
        Collapsed U: ONE `posterior_rollout_grouped_summary` call with G = S and the model shared by the groups.  Explicit U:
        `kernel_pre_cal` once, then `rollout_grouped_summary` with the shared U and no q_sqrt.
        `eps` (len(Y_test), S, num_per_chain, D) injects the draws of base_model.py:306 (else numpy's default_rng(seed): the model's
        own generator is not advanced).  Parameters newer on the device than on the host are pulled first.
        method "moment" replaces the rollouts by the moment-matched prediction (`predict_moments`): deterministic, one pass of
        len(Y_test) launches; num_per_chain, eps and seed are ignored, and predict_y_var equals predict_y_var_total.
        Returns a dict: RMSE (first 30 test points, base_model.py:346-348), ll (mean log predictive density), ll_original_units,
        and the per-step arrays predict_y, predict_y_var, predict_y_var_total, lpd, lpd_gauss."""
        from . import conditionals_multi_output as cmo
        from .prediction import posterior_rollout_grouped_summary, rollout_grouped_summary
        if method not in ("rollouts", "moment"):
            raise ValueError(f"evaluate_heldout: method: expected 'rollouts' or 'moment', got {method!r}")
        Y_test = np.asarray(Y_test, dtype=np.float64)
        if Y_test.ndim == 1:
            Y_test = Y_test[:, None]
        if Y_test.ndim != 2 or Y_test.shape[0] < 1 or Y_test.shape[1] != self.Y.shape[1]:
            raise ValueError(f"evaluate_heldout: Y_test: expected (n_test >= 1, {self.Y.shape[1]}), got {Y_test.shape}")
        if method == "moment":
            out = self.predict_moments(control_inputs, Y_test.shape[0], Y_test=Y_test, Y_train_std=Y_train_std)
            return {k: v for k, v in out.items() if k not in ("m_x", "S_x")}          # the keys of the default method
        if self._host_stale:
            self.pull_parameters()
        S, D, R, steps = self.num_chains, self.output_dim, int(num_per_chain), Y_test.shape[0]
        if R < 1:
            raise ValueError("num_per_chain must be at least 1")
        ci = self.control_inputs if control_inputs is None else np.asarray(control_inputs, dtype=np.float64)
        if eps is None:
            eps = np.random.default_rng(seed).standard_normal((steps, S, R, D))
        eps = np.asarray(eps, dtype=np.float64)
        if eps.shape != (steps, S, R, D):
            raise ValueError(f"eps: expected {(steps, S, R, D)}, got {eps.shape}")
        lay, lik, n_train = self.layers[-1], self.likelihood, self.Y.shape[0]
        if self.U_collapse:
            return posterior_rollout_grouped_summary(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train,
                                                     steps, eps, lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        return rollout_grouped_summary([Lm] * S, [lay.Z] * S, [lay.kernel] * S, [lay.U] * S, None,
                                       [self._X_chains[s_][-1] for s_ in range(S)], ci, n_train, steps, [self.Q] * S, eps,
                                       lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std)

    def predict_moments(self, control_inputs, test_len, *, Y_test=None, Y_train_std=1.0, q_mode="reference"):
        """Moment-matched held-out prediction: from every chain's X_s[-1] with zero start covariance, the Gaussian state is pushed
        test_len steps through the learned transition in closed form (prediction.moment_grouped has the method; SquaredExponential
        kernels only) and summarised on the device (prediction.moment_summary has the quantities) -- deterministic, no rollouts.
        Collapsed U: ONE `posterior_moment_grouped_summary` call with G = S and the model shared by the groups; q_mode as
        `predict_transition`.  Explicit U: `kernel_pre_cal` once, then `moment_grouped_summary` with the shared U and no q_sqrt.
        control_inputs None: the model's own; rows [n_train, n_train + test_len) feed the steps.  Parameters newer on the device
        than on the host are pulled first.
        Returns the dict of `evaluate_heldout` (without Y_test: predict_y, predict_y_var, predict_y_var_total only) plus m_x
        (S, test_len, D) and S_x (S, test_len, D, D), the state moments of every chain."""
        from . import conditionals_multi_output as cmo
        from .prediction import moment_grouped_summary, posterior_moment_grouped_summary
        if q_mode not in cmo.Q_MODES:
            raise ValueError(f"predict_moments: q_mode: expected one of {sorted(cmo.Q_MODES)}, got {q_mode!r}")
        steps = int(test_len)
        if steps < 1:
            raise ValueError("predict_moments: test_len must be at least 1")
        if self._host_stale:
            self.pull_parameters()
        S = self.num_chains
        ci = self.control_inputs if control_inputs is None else np.asarray(control_inputs, dtype=np.float64)
        lay, lik, n_train = self.layers[-1], self.likelihood, self.Y.shape[0]
        if self.U_collapse:
            return posterior_moment_grouped_summary(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train,
                                                    steps, lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std, q_mode=q_mode,
                                                    return_moments=True)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        return moment_grouped_summary(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [self._X_chains[s_][-1] for s_ in range(S)], ci,
                                      n_train, steps, self.Q, lik.CC, lik.DD, lik.log_Rchols, Y_test, Y_train_std, q_mode=q_mode,
                                      return_moments=True)

    def _heldout_record(self, who, Y_test, control_inputs, x0, S0, q_mode):
        """What `filter_heldout` and `forecast_heldout` do before their call: q_mode and Y_test (len, Ydim) checked, parameters newer
        on the device pulled, the start broadcast to the chains (None stays None), the control inputs chosen.  (Called through the
        class: the argument tests hand the two methods a stand-in for the model.)"""
        from . import conditionals_multi_output as cmo
        if q_mode not in cmo.Q_MODES:
            raise ValueError(f"{who}: q_mode: expected one of {sorted(cmo.Q_MODES)}, got {q_mode!r}")
        Y_test = np.asarray(Y_test, dtype=np.float64)
        if Y_test.ndim == 1:
            Y_test = Y_test[:, None]
        if Y_test.ndim != 2 or Y_test.shape[1] != self.Y.shape[1]:
            raise ValueError(f"{who}: Y_test: expected (n_test, {self.Y.shape[1]}), got {Y_test.shape}")
        if self._host_stale:
            self.pull_parameters()
        S, D = self.num_chains, self.output_dim
        x0s = None if x0 is None else np.broadcast_to(np.asarray(x0, dtype=np.float64), (S, D))
        S0s = None if S0 is None else np.broadcast_to(np.asarray(S0, dtype=np.float64), (S, D, D))
        ci = self.control_inputs if control_inputs is None else np.asarray(control_inputs, dtype=np.float64)
        return Y_test, x0s, S0s, ci

    def filter_heldout(self, Y_test, control_inputs=None, *, x0=None, S0=None, smooth=False, q_mode="reference", Y_train_std=1.0):
        """One-step-ahead (prequential) evaluation, filtered and (with `smooth`) smoothed latent states of a held-out record: every
        chain's Gaussian state is pushed through the learned transition and updated with each row of Y_test (len, Ydim; a NaN entry
        is unobserved, trailing all-NaN rows forecast) -- prediction.filter_grouped has the method and the dict that is returned
        (SquaredExponential kernels only; deterministic).  x0 None: every chain starts at its X_s[-1] (the record continues the
        training sequence) with S0 None: zero covariance; else x0 (D,) or (S, D) and S0 (D, D) or (S, D, D) for a fresh record.
        Collapsed U: ONE `posterior_filter_grouped` call with G = S and the model shared by the groups.  Explicit U:
        `kernel_pre_cal` once, then `filter_grouped` with the shared U and no q_sqrt.  control_inputs None: the model's own; rows
        [n_train, n_train + len(Y_test)) feed the steps, as in `predict_moments`.  Parameters newer on the device than on the host
        are pulled first."""
        return DGPSSM._filter_heldout(self, "filter_heldout", "moment", Y_test, control_inputs, x0, S0, smooth, q_mode, Y_train_std)

    def filter_heldout_linearised(self, Y_test, control_inputs=None, *, x0=None, S0=None, smooth=False, q_mode="reference",
                                  Y_train_std=1.0):
        """`filter_heldout` with the linearised (extended Kalman) rule in place of moment matching: the same arguments, the same
        dict, the same two forms, with method="linearised" of prediction.filter_grouped / posterior_filter_grouped -- every chain's
        transition is linearised at its filtered mean.  Much cheaper per row of the record; first order in the state covariance where
        moment matching is exact for the Gaussian ("Linearised filtering", has both the speed and the fit).  A
        method of its own: the parameter list of `filter_heldout` is pinned."""
        return DGPSSM._filter_heldout(self, "filter_heldout_linearised", "linearised", Y_test, control_inputs, x0, S0, smooth, q_mode,
                                      Y_train_std)

    def _filter_heldout(self, who, method, Y_test, control_inputs, x0, S0, smooth, q_mode, Y_train_std):
        """The body of `filter_heldout` and `filter_heldout_linearised` (called through the class, as `_heldout_record`)."""
        from . import conditionals_multi_output as cmo
        from .prediction import _filter_method, filter_grouped, posterior_filter_grouped
        _filter_method(who, method)
        Y_test, x0s, S0s, ci = DGPSSM._heldout_record(self, who, Y_test, control_inputs, x0, S0, q_mode)
        S, lay, lik, n_train = self.num_chains, self.layers[-1], self.likelihood, self.Y.shape[0]
        if self.U_collapse:
            return posterior_filter_grouped(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train, Y_test,
                                            lik.CC, lik.DD, lik.log_Rchols, x0s=x0s, S0s=S0s, q_mode=q_mode, smooth=smooth,
                                            Y_train_std=Y_train_std, method=method)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        starts = [self._X_chains[s_][-1] for s_ in range(S)] if x0s is None else list(x0s)
        return filter_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, starts, ci, n_train, Y_test, self.Q, lik.CC, lik.DD,
                              lik.log_Rchols, S0s=S0s, q_mode=q_mode, smooth=smooth, Y_train_std=Y_train_std, method=method)

    def filter_records(self, Y_records, control_records=None, *, lengths=None, x0=None, S0=None, smooth=False, q_mode="reference",
                       Y_train_std=1.0, records_per_pass=0):
        """`filter_heldout_linearised` over R held-out records -- trials, segments, cross-validation folds -- in ONE call: every
        (chain, record) pair is an independent linearised filter with the observations Y_records[r] (Y_records (R, steps, Ydim), NaN =
        unobserved), the control rows control_records[r] ((R, steps, C); a model with controls needs them: a fresh trial has no
        natural default) and its own start -- prediction.filter_records_grouped has the method, `lengths` for records of different
        length, and the dict that is returned (per-record scalars as arrays (R,), ll_all over all records).  x0 None: every record
        starts at its chain's X_s[-1] with S0 None: zero covariance; else x0 (D,), (R, D) or (S, R, D) and S0 (D, D), (R, D, D) or
        (S, R, D, D).  Collapsed U: ONE `posterior_filter_records_grouped` call with G = S and the model shared by the groups.
        Explicit U: `kernel_pre_cal` once, then `filter_records_grouped` with the shared U and no q_sqrt.  Parameters newer on the
        device than on the host are pulled first.  SquaredExponential kernels only; deterministic."""
        return DGPSSM._filter_records(self, "filter_records", "filter_records_grouped", Y_records, control_records, lengths, x0, S0, smooth,
                                      q_mode, Y_train_std, records_per_pass)

    def filter_records_cubature(self, Y_records, control_records=None, *, lengths=None, x0=None, S0=None, smooth=False, q_mode="reference",
                                Y_train_std=1.0, records_per_pass=0):
        """`filter_records` with the third-degree spherical cubature rule in place of the linearisation: 2D sigma points per step, a
        one-step difference from moment matching that is second order in the state covariance where the linearised rule's is first
        order -- the call for a caller who needs the latent states themselves (smoothing, control) over many records, or over one:
        R = 1 is a valid single-record call.  prediction.filter_cubature_records_grouped has the method.  Parameters, checks, the two
        forms (collapsed U: ONE `posterior_filter_cubature_records_grouped` call; explicit U: `kernel_pre_cal` once, then
        `filter_cubature_records_grouped`) and the dict that is returned are those of `filter_records`."""
        return DGPSSM._filter_records(self, "filter_records_cubature", "filter_cubature_records_grouped", Y_records, control_records, lengths,
                                      x0, S0, smooth, q_mode, Y_train_std, records_per_pass)

    def filter_records_particle(self, Y_records, control_records=None, *, num_particles=256, lengths=None, x0=None, S0=None,
                                q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared", return_particles=False):
        """`filter_records` with a bootstrap particle filter of `num_particles` particles per (chain, record) in place of a Gaussian
        rule: the arbiter of the three Gaussian filters -- exact as the particle count grows, with the unbiased SMC estimate
        `log_evidence` (S, R) of the held-out evidence and the effective sample size `ess` per row.
        prediction.filter_particle_records_grouped has the method and the dict that is returned (no smoothing: particle smoothing is
        not built into this call, `smooth_records_particle` has it).  The draws come from np.random.default_rng(seed), or from the model's own generator when seed is None.  noise:
        "shared" -- one set of draws (steps, N, D) for every chain and record (common random numbers; each track's estimator stays
        unbiased); "per_record" -- one set per record, shared by the chains; "independent" -- one per (chain, record), refused with
        the byte count when the draws would exceed 1 GiB.  The checks, the start (x0, S0) and the two forms (collapsed U: ONE
        `posterior_filter_particle_records_grouped` call; explicit U: `kernel_pre_cal` once, then `filter_particle_records_grouped`)
        are `filter_records`'; R = 1 is a valid single-record call."""
        return DGPSSM._records_particle(self, "filter_records_particle", "filter_particle_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles)

    def filter_records_adapted(self, Y_records, control_records=None, *, num_particles=256, lengths=None, x0=None, S0=None,
                               q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared", return_particles=False):
        """`filter_records_particle` with the optimal proposal in place of the bootstrap one (the fully adapted auxiliary particle
        filter): the parents are weighted by how well they predict the row before anything is drawn, so the filter does not collapse
        where the observations are informative.  The parameters, the checks, the draws (the same seed gives the same draws in the same
        order) and the two forms (collapsed U: ONE `posterior_filter_adapted_records_grouped` call; explicit U: `kernel_pre_cal` once,
        then `filter_adapted_records_grouped`) are `filter_records_particle`'s; prediction.filter_adapted_records_grouped has the
        method and the dict that is returned: particles[t] is the equally weighted filtered set after row t (not X^-) and
        ancestors[t, i] indexes the set carried into row t.  Smoothing and joint trajectories on the adapted sets are
        `smooth_records_adapted` and `sample_records_adapted`; there are no forecasts on them."""
        return DGPSSM._records_particle(self, "filter_records_adapted", "filter_adapted_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles)

    def smooth_records_particle(self, Y_records, control_records=None, *, num_particles=256, lengths=None, x0=None, S0=None,
                                q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared", return_particles=False):
        """`filter_records_particle` followed by the marginal particle smoother of every (chain, record) track in the same call: the
        arbiter of the three Gaussian smoothers.  The parameters, the checks, the draw generation (the same seed gives the same
        filter, bit for bit) and the two forms (collapsed U: ONE `posterior_smooth_particle_records_grouped` call; explicit U:
        `kernel_pre_cal` once, then `smooth_particle_records_grouped`) are `filter_records_particle`'s;
        prediction.smooth_particle_records_grouped has the method and the dict that is returned: the filter's, plus m_smooth, S_smooth
        and ess_smooth (S, R, steps, ...), with return_particles also weights, w_smooth, trans_mean and trans_var."""
        return DGPSSM._records_particle(self, "smooth_records_particle", "smooth_particle_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles)

    def sample_records_particle(self, Y_records, control_records=None, *, num_particles=256, num_trajectories=64, lengths=None, x0=None,
                                S0=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared",
                                return_particles=False):
        """`filter_records_particle` followed by the backward simulation of `num_trajectories` joint smoothed trajectories of every
        (chain, record) track in the same call: draws of whole paths given the whole record, for statistics that the marginal
        smoother of `smooth_records_particle` cannot give (excursions, first-passage times, sums over a window, the lag-one
        covariance).  The parameters, the checks and the two forms (collapsed U: ONE `posterior_backsim_particle_records_grouped`
        call; explicit U: `kernel_pre_cal` once, then `backsim_particle_records_grouped`) are `filter_records_particle`'s.  The
        filter's draws are drawn first and in `filter_records_particle`'s order, so the same seed gives the same filter, bit for bit;
        the uniforms of the backward simulation (steps, num_trajectories), with the leading dimensions of `noise`, are drawn after
        them.  prediction.backsim_particle_records_grouped has the method and the dict that is returned: the filter's, plus
        trajectories (S, R, B, steps, D), traj_index (S, R, steps, B), m_traj, S_traj and lag_cov, with return_particles also weights,
        trans_mean and trans_var."""
        B = num_trajectories
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= B <= 4096:
            raise ValueError(f"sample_records_particle: num_trajectories: expected an integer in [1, 4096], got {num_trajectories!r}")
        return DGPSSM._records_particle(self, "sample_records_particle", "backsim_particle_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles,
                                        int(B))

    def smooth_records_adapted(self, Y_records, control_records=None, *, num_particles=256, lengths=None, x0=None, S0=None,
                               q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared", return_particles=False):
        """`filter_records_adapted` followed by the marginal particle smoother of every (chain, record) track on the adapted sets in
        the same call: the smoother to use where the observations are informative and `smooth_records_particle` inherits the
        bootstrap filter's collapsed sets.  The parameters, the checks, the draw generation (the same seed gives
        `filter_records_adapted`'s draws, hence its filter bit for bit) and the two forms (collapsed U: ONE
        `posterior_smooth_adapted_records_grouped` call; explicit U: `kernel_pre_cal` once, then `smooth_adapted_records_grouped`)
        are `filter_records_particle`'s; prediction.smooth_adapted_records_grouped has the method and the dict that is returned: the
        adapted filter's, plus m_smooth, S_smooth and ess_smooth (S, R, steps, ...), with return_particles also w_smooth, trans_mean
        and trans_var (no weights: the filtered sets are equally weighted)."""
        return DGPSSM._records_particle(self, "smooth_records_adapted", "smooth_adapted_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles)

    def sample_records_adapted(self, Y_records, control_records=None, *, num_particles=256, num_trajectories=64, lengths=None, x0=None,
                               S0=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared",
                               return_particles=False):
        """`filter_records_adapted` followed by the backward simulation of `num_trajectories` joint smoothed trajectories of every
        (chain, record) track on the adapted sets in the same call: `sample_records_particle` on the filter that does not collapse.
        The parameters, the checks and the two forms (collapsed U: ONE `posterior_backsim_adapted_records_grouped` call; explicit U:
        `kernel_pre_cal` once, then `backsim_adapted_records_grouped`) are `sample_records_particle`'s.  The filter's draws are drawn
        first and in `filter_records_adapted`'s order, so the same seed gives the same filter, bit for bit; the uniforms of the
        backward simulation (steps, num_trajectories), with the leading dimensions of `noise`, are drawn after them.
        prediction.backsim_adapted_records_grouped has the method and the dict that is returned: the adapted filter's, plus
        trajectories (S, R, B, steps, D), traj_index (S, R, steps, B), m_traj, S_traj and lag_cov, with return_particles also
        trans_mean and trans_var."""
        B = num_trajectories
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= B <= 4096:
            raise ValueError(f"sample_records_adapted: num_trajectories: expected an integer in [1, 4096], got {num_trajectories!r}")
        return DGPSSM._records_particle(self, "sample_records_adapted", "backsim_adapted_records_grouped", Y_records, control_records,
                                        num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles,
                                        int(B))

    def filter_records_adaptive(self, Y_records, control_records=None, *, num_particles=256, ess_threshold=0.5, lengths=None, x0=None,
                                S0=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0, seed=None, noise="shared", draws="numpy",
                                return_particles=False):
        """`filter_records_particle` with ADAPTIVE resampling: every (chain, record) track carries a weighted set and resamples only
        on the rows whose effective sample size falls below ess_threshold * num_particles -- the textbook form, for records whose rows
        have few or uninformative outputs, where resampling at every row only adds variance.  ess_threshold: a finite number >= 0
        (0 never resamples; above 1 always, which is `filter_records_particle` bit for bit).  draws="numpy": the draws of
        `filter_records_particle` for the same seed (np.random.default_rng(seed), or the model's generator), with its `noise` modes and
        its 1 GiB refusal; draws="device": generated on the device as in `particle_records_seeded`, which needs an integer seed in
        [0, 2^64).  The checks, the start and the two forms (collapsed U: ONE `posterior_filter_adaptive_records_grouped` /
        `posterior_adaptive_records_seeded` call; explicit U: `kernel_pre_cal` once, then `filter_adaptive_records_grouped` /
        `adaptive_records_seeded`) are `filter_records`'; prediction.filter_adaptive_records_grouped has the method and the dict that
        is returned: the bootstrap call's plus resampled (S, R, steps) and, with return_particles, weights (S, R, steps, N)."""
        from . import prediction as pr
        who = "filter_records_adaptive"
        if not isinstance(draws, str) or draws not in ("numpy", "device"):
            raise ValueError(f"{who}: draws: expected \"numpy\" or \"device\", got {draws!r}")
        thr = pr._ess_threshold(who, ess_threshold)
        if draws == "numpy":
            return DGPSSM._records_particle(self, who, "filter_adaptive_records_grouped", Y_records, control_records, num_particles, lengths,
                                            x0, S0, q_mode, Y_train_std, records_per_pass, seed, noise, return_particles,
                                            extra=dict(ess_threshold=thr))
        if not pr._is_int(seed):
            raise ValueError(f"{who}: seed: draws=\"device\" needs an integer seed in [0, 2^64), got {seed!r}")
        shape = np.shape(Y_records)
        if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{who}: Y_records: expected (R, steps, {self.Y.shape[1]}), got {shape}")
        pr._pack_seeded(who, self.num_chains, shape[0], shape[1], self.output_dim, num_particles, "bootstrap", "filter", seed, noise, 0,
                        return_particles)
        seeded = dict(num_particles=num_particles, ess_threshold=thr, seed=seed, noise=noise, return_particles=return_particles)
        return DGPSSM._filter_records(self, who, "adaptive_records_seeded", Y_records, control_records, lengths, x0, S0, None, q_mode,
                                      Y_train_std, records_per_pass, seeded=seeded)

    def _records_particle(self, who, fn, Y_records, control_records, num_particles, lengths, x0, S0, q_mode, Y_train_std, records_per_pass,
                          seed, noise, return_particles, num_trajectories=None, extra=None):
        """The body of `filter_records_particle`, `smooth_records_particle` and `sample_records_particle`: the checks and the draws,
        then `_filter_records`.  num_trajectories: the uniforms of the backward simulation are drawn after the filter's draws.
        extra: further keywords of the prediction-level function (`filter_records_adaptive`'s ess_threshold)."""
        if noise not in ("shared", "per_record", "independent"):
            raise ValueError(f"{who}: noise: expected \"shared\", \"per_record\" or \"independent\", got {noise!r}")
        N = num_particles
        if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or not 2 <= N <= 2048:
            raise ValueError(f"{who}: num_particles: expected an integer in [2, 2048], got {num_particles!r}")
        shape = np.shape(Y_records)
        if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{who}: Y_records: expected (R, steps, {self.Y.shape[1]}), got {shape}")
        S, D, (R, steps) = self.num_chains, self.output_dim, shape[:2]
        lead = {"shared": (), "per_record": (R,), "independent": (S, R)}[noise]
        nbytes = 8 * int(np.prod(lead, dtype=np.int64)) * (steps * N * D + steps + (N * D if S0 is not None else 0))
        if noise == "independent" and nbytes > 2 ** 30:
            raise ValueError(f"{who}: noise=\"independent\" needs {nbytes} bytes of draws, more than 1 GiB: use \"per_record\" or \"shared\"")
        rng = np.random.default_rng(seed) if seed is not None else self._rng
        draws = dict(eps=rng.standard_normal(lead + (steps, N, D)), unif=rng.random(lead + (steps,)),
                     xi0=None if S0 is None else rng.standard_normal(lead + (N, D)), return_particles=return_particles)
        if num_trajectories is not None:
            draws["unif_bs"] = rng.random(lead + (steps, num_trajectories))
        if extra:
            draws["extra"] = extra
        return DGPSSM._filter_records(self, who, fn, Y_records, control_records, lengths, x0, S0, None, q_mode,
                                      Y_train_std, records_per_pass, draws)

    def particle_records_seeded(self, Y_records, control_records=None, *, rule="bootstrap", stage="filter", num_particles=256,
                                num_trajectories=0, lengths=None, x0=None, S0=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0,
                                seed=None, noise="shared", return_particles=False):
        """The six particle methods above with the draws generated on the DEVICE from a seed instead of by NumPy on the host:
        rule "bootstrap" / "adapted" and stage "filter" / "smooth" / "backsim" select `filter_records_particle`,
        `smooth_records_particle`, `sample_records_particle` (num_trajectories, with stage="backsim" only) or their adapted
        siblings, whose other parameters, checks, two forms (collapsed U: ONE `posterior_particle_records_seeded` call; explicit U:
        `kernel_pre_cal` once, then `particle_records_seeded`) and returned dict these are.  Nothing is generated, scanned or
        uploaded by the host, so the 1 GiB refusal of noise="independent" does not apply: the library's own index limit
        (S * R * steps * N * D < 2^31) does, with its message.  seed: an integer in [0, 2^64); None takes one 64-bit integer from the
        model's generator.  The streams are Philox4x32-10, not NumPy's: the same seed does NOT reproduce `filter_records_particle`'s
        draws, it reproduces this method's, whatever the number of chains and records and records_per_pass are
        (prediction.particle_draws returns them; DESIGN.md section 9, "Device draws").  A method of its own: the parameter lists of
        the six methods above are pinned."""
        from . import prediction as pr
        who = "particle_records_seeded"
        if seed is None:
            seed = int(self._rng.integers(0, 2 ** 64, dtype=np.uint64))
        shape = np.shape(Y_records)
        if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{who}: Y_records: expected (R, steps, {self.Y.shape[1]}), got {shape}")
        pr._pack_seeded(who, self.num_chains, shape[0], shape[1], self.output_dim, num_particles, rule, stage, seed, noise, num_trajectories,
                        return_particles)
        seeded = dict(rule=rule, stage=stage, num_particles=num_particles, num_trajectories=num_trajectories, seed=seed, noise=noise,
                      return_particles=return_particles)
        return DGPSSM._filter_records(self, who, who, Y_records, control_records, lengths, x0, S0, None, q_mode, Y_train_std,
                                      records_per_pass, seeded=seeded)

    def _filter_records(self, who, fn, Y_records, control_records, lengths, x0, S0, smooth, q_mode, Y_train_std, records_per_pass, draws=None,
                        seeded=None):
        """The body of `filter_records`, `filter_records_cubature` and `filter_records_particle` (called through the class, as
        `_filter_heldout`): `fn` names the prediction-level function of the explicit form, "posterior_" + fn the fused one; draws: the
        particle filter's eps, unif, xi0 and return_particles (it has no `smooth`); seeded: the keywords of `particle_records_seeded`
        in their place."""
        from . import conditionals_multi_output as cmo
        from . import prediction as pr
        if q_mode not in cmo.Q_MODES:
            raise ValueError(f"{who}: q_mode: expected one of {sorted(cmo.Q_MODES)}, got {q_mode!r}")
        Y = np.asarray(Y_records, dtype=np.float64)
        if Y.ndim != 3 or Y.shape[0] < 1 or Y.shape[2] != self.Y.shape[1]:
            raise ValueError(f"{who}: Y_records: expected (R, steps, {self.Y.shape[1]}), got {Y.shape}")
        if self._host_stale:
            self.pull_parameters()
        S, D, R = self.num_chains, self.output_dim, Y.shape[0]
        lay, lik = self.layers[-1], self.likelihood
        C = np.shape(lay.Z)[1] - D
        if C > 0 and control_records is None:
            raise ValueError(f"{who}: control_records: the model has {C} control columns and a fresh record has no default, expected "
                             f"({R}, {Y.shape[1]}, {C})")

        def spread(v, tail, name):                                # tail, (R,) + tail or (S, R) + tail -> (S, R) + tail
            if v is None:
                return None
            v = np.asarray(v, dtype=np.float64)
            if v.shape not in (tail, (R,) + tail, (S, R) + tail):
                raise ValueError(f"{who}: {name}: expected {tail}, {(R,) + tail} or {(S, R) + tail}, got {v.shape}")
            return np.broadcast_to(v, (S, R) + tail)
        x0s, S0s = spread(x0, (D,), "x0"), spread(S0, (D, D), "S0")
        kw = dict(lengths=lengths, S0s=S0s, q_mode=q_mode, smooth=smooth, Y_train_std=Y_train_std, records_per_pass=records_per_pass)
        tail = ()
        if draws is not None:                                     # the particle filter: eps and unif follow log_Rchols, no `smooth`
            del kw["smooth"]
            tail = (draws["eps"], draws["unif"]) + ((draws["unif_bs"],) if "unif_bs" in draws else ())
            kw.update(xi0=draws["xi0"], return_particles=draws["return_particles"], **draws.get("extra", {}))
        if seeded is not None:                                    # the draws are the device's: nothing follows log_Rchols, no `smooth`
            del kw["smooth"]
            kw.update(seeded)
        if self.U_collapse:
            return getattr(pr, "posterior_" + fn)(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, self.control_inputs,
                                                  control_records, Y, lik.CC, lik.DD, lik.log_Rchols, *tail, x0s=x0s, **kw)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        if x0s is None:
            x0s = np.broadcast_to(np.stack([self._X_chains[s_][-1] for s_ in range(S)])[:, None, :], (S, R, D))
        return getattr(pr, fn)(Lm, lay.Z, lay.kernel, [lay.U] * S, None, x0s, control_records, Y, self.Q, lik.CC, lik.DD, lik.log_Rchols, *tail,
                               **kw)

    def forecast_heldout(self, Y_test, control_inputs=None, horizon=10, *, stride=1, origins=None, x0=None, S0=None, q_mode="reference",
                         Y_train_std=1.0, return_tracks=False):
        """k-step-ahead evaluation of a held-out record for k = 1 .. horizon, with every row of the record as the forecast origin
        (every `stride`-th, or the rows `origins`): the filter of `filter_heldout`, then from each origin `horizon` steps of the
        moment-matched prediction started at the filtered state -- prediction.forecast_grouped has the method and the dict that is
        returned (the horizon curves rmse_h, ll_h, ll_gauss_h, n_h of shape (horizon, Ydim) among it; SquaredExponential kernels
        only; deterministic).  The start, the control rows and the two forms (collapsed U: ONE `posterior_forecast_grouped` call;
        explicit U: `kernel_pre_cal` once, then `forecast_grouped`) are those of `filter_heldout`."""
        return DGPSSM._forecast_heldout(self, "forecast_heldout", "moment", Y_test, control_inputs, horizon, stride, origins, x0, S0, q_mode,
                                        Y_train_std, return_tracks)

    def forecast_heldout_linearised(self, Y_test, control_inputs=None, horizon=10, *, stride=1, origins=None, x0=None, S0=None,
                                    q_mode="reference", Y_train_std=1.0, return_tracks=False):
        """`forecast_heldout` with the linearised (extended Kalman) rule for the filter and for the tracks: the same arguments, the
        same dict, the same two forms, through prediction.posterior_forecast_linear_grouped / forecast_linear_grouped -- the filter
        of `filter_heldout_linearised`, then from each origin `horizon` steps of the same linearisation without a measurement update
        ("Linearised forecasts", has both the speed and the fit).  A method of its own: the parameter list of
        `forecast_heldout` is pinned."""
        return DGPSSM._forecast_heldout(self, "forecast_heldout_linearised", "linearised", Y_test, control_inputs, horizon, stride, origins,
                                        x0, S0, q_mode, Y_train_std, return_tracks)

    def forecast_heldout_cubature(self, Y_test, control_inputs=None, horizon=10, *, stride=1, origins=None, x0=None, S0=None,
                                  q_mode="reference", Y_train_std=1.0, return_tracks=False):
        """`forecast_heldout` with the third-degree spherical cubature rule for the filter and for the tracks: the same arguments, the
        same dict, the same two forms, through prediction.posterior_forecast_cubature_grouped / forecast_cubature_grouped -- the filter
        of `filter_records_cubature` over the one record, then from each origin `horizon` steps of the same 2D-point propagation
        without a measurement update ("Cubature forecasts", has both the speed and the fit)."""
        return DGPSSM._forecast_heldout(self, "forecast_heldout_cubature", "cubature", Y_test, control_inputs, horizon, stride, origins,
                                        x0, S0, q_mode, Y_train_std, return_tracks)

    def forecast_heldout_particle(self, Y_test, control_inputs=None, horizon=10, *, num_particles=256, seed=None, noise="shared", stride=1,
                                  origins=None, x0=None, S0=None, q_mode="reference", Y_train_std=1.0, return_tracks=False):
        """`forecast_heldout` by particles: the bootstrap particle filter of `filter_records_particle` over the one record, then from
        each origin `horizon` steps of `num_particles` equally weighted particles per (chain, origin), started from the set the filter
        carries after that row and advanced without weighting or resampling -- the arbiter of the three Gaussian fans at every
        horizon: ll_h is the density of the mixture of all S N particles' emissions and is directly comparable with theirs.
        prediction.forecast_particle_grouped has the method and the dict that is returned (lpd_fc (S, B, horizon, Ydim) among it).
        The draws come from np.random.default_rng(seed), or from the model's own generator when seed is None, as
        `filter_records_particle` generates them.  noise: "shared" -- one set of filter draws for every chain and one set of forecast
        draws (horizon, N, D) for every chain and origin (common random numbers); "independent" -- one set per chain, and per
        (chain, origin) for the forecast draws, refused with the byte count when the draws would exceed 1 GiB.  The other parameters,
        the start, the control rows and the two forms (collapsed U: ONE `posterior_forecast_particle_grouped` call; explicit U:
        `kernel_pre_cal` once, then `forecast_particle_grouped`) are those of `forecast_heldout`."""
        return DGPSSM._forecast_heldout_particles(self, "forecast_heldout_particle", False, Y_test, control_inputs, horizon, num_particles,
                                                  seed, noise, stride, origins, x0, S0, q_mode, Y_train_std, return_tracks)

    def forecast_heldout_adapted(self, Y_test, control_inputs=None, horizon=10, *, num_particles=256, seed=None, noise="shared", stride=1,
                                 origins=None, x0=None, S0=None, q_mode="reference", Y_train_std=1.0, return_tracks=False):
        """`forecast_heldout_particle` on the sets of the fully adapted particle filter (`filter_records_adapted`'s rule over the one
        record): each track starts from the equally weighted filtered set after its origin, and every forecast row is the adapted
        filter's Rao-Blackwellised prediction (the last step's process noise in closed form), so the row k = 1 from origin o is the
        filter's own one-step prediction of row o + 1.  prediction.forecast_adapted_grouped has the method.  The parameters, the
        draws (the same `seed` gives the same draws as `forecast_heldout_particle`), the two forms (collapsed U: ONE
        `posterior_forecast_adapted_grouped` call; explicit U: `kernel_pre_cal` once, then `forecast_adapted_grouped`) and the keys of
        the returned dict are that method's."""
        return DGPSSM._forecast_heldout_particles(self, "forecast_heldout_adapted", True, Y_test, control_inputs, horizon, num_particles,
                                                  seed, noise, stride, origins, x0, S0, q_mode, Y_train_std, return_tracks)

    def _forecast_heldout_particles(self, who, adapted, Y_test, control_inputs, horizon, num_particles, seed, noise, stride, origins, x0, S0,
                                    q_mode, Y_train_std, return_tracks, return_particles=False):
        """The body of `forecast_heldout_particle` and `forecast_heldout_adapted` (called through the class, as `_heldout_record`);
        return_particles: `forecast_scores` asks for fc_particles as well."""
        from . import conditionals_multi_output as cmo
        from . import prediction as pr
        fused, explicit = ((pr.posterior_forecast_adapted_grouped, pr.forecast_adapted_grouped) if adapted else
                           (pr.posterior_forecast_particle_grouped, pr.forecast_particle_grouped))
        if noise not in ("shared", "independent"):
            raise ValueError(f"{who}: noise: expected \"shared\" or \"independent\", got {noise!r}")
        N = num_particles
        if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or not 2 <= N <= 2048:
            raise ValueError(f"{who}: num_particles: expected an integer in [2, 2048], got {num_particles!r}")
        Y_test, x0s, S0s, ci = DGPSSM._heldout_record(self, who, Y_test, control_inputs, x0, S0, q_mode)
        S, D, steps = self.num_chains, self.output_dim, Y_test.shape[0]
        h, org = pr._pack_forecast(who, steps, horizon, origins, stride)
        B = len(org)
        lead, lead_fc = ((), ()) if noise == "shared" else ((S,), (S, B))
        nbytes = 8 * (int(np.prod(lead, dtype=np.int64)) * (steps * N * D + steps + (N * D if S0 is not None else 0)) +
                      int(np.prod(lead_fc, dtype=np.int64)) * h * N * D)
        if noise == "independent" and nbytes > 2 ** 30:
            raise ValueError(f"{who}: noise=\"independent\" needs {nbytes} bytes of draws, more than 1 GiB: use \"shared\"")
        rng = np.random.default_rng(seed) if seed is not None else self._rng
        eps, unif = rng.standard_normal(lead + (steps, N, D)), rng.random(lead + (steps,))
        xi0 = None if S0 is None else rng.standard_normal(lead + (N, D))
        eps_fc = rng.standard_normal(lead_fc + (h, N, D))
        lay, lik, n_train = self.layers[-1], self.likelihood, self.Y.shape[0]
        kw = dict(xi0=xi0, origins=org, S0s=S0s, q_mode=q_mode, Y_train_std=Y_train_std, return_tracks=return_tracks)
        if return_particles:
            kw["return_particles"] = True
        if self.U_collapse:
            return fused(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train, Y_test, lik.CC, lik.DD,
                         lik.log_Rchols, h, eps, unif, eps_fc, x0s=x0s, **kw)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        starts = [self._X_chains[s_][-1] for s_ in range(S)] if x0s is None else list(x0s)
        return explicit(Lm, lay.Z, lay.kernel, [lay.U] * S, None, starts, ci, n_train, Y_test, self.Q, lik.CC, lik.DD, lik.log_Rchols, h,
                        eps, unif, eps_fc, **kw)

    def _forecast_heldout(self, who, method, Y_test, control_inputs, horizon, stride, origins, x0, S0, q_mode, Y_train_std, return_tracks):
        """The body of `forecast_heldout`, `forecast_heldout_linearised` and `forecast_heldout_cubature` (called through the class, as
        `_heldout_record`)."""
        from . import conditionals_multi_output as cmo
        from . import prediction as pr
        rules = {"moment": (pr.posterior_forecast_grouped, pr.forecast_grouped),
                 "linearised": (pr.posterior_forecast_linear_grouped, pr.forecast_linear_grouped),
                 "cubature": (pr.posterior_forecast_cubature_grouped, pr.forecast_cubature_grouped)}
        if method not in rules:
            raise ValueError(f"{who}: method: expected one of {list(rules)}, got {method!r}")
        fused, explicit = rules[method]
        Y_test, x0s, S0s, ci = DGPSSM._heldout_record(self, who, Y_test, control_inputs, x0, S0, q_mode)
        S, lay, lik, n_train = self.num_chains, self.layers[-1], self.likelihood, self.Y.shape[0]
        kw = dict(origins=origins, stride=stride, S0s=S0s, q_mode=q_mode, Y_train_std=Y_train_std, return_tracks=return_tracks)
        if self.U_collapse:
            return fused(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q, ci, n_train, Y_test, lik.CC, lik.DD,
                         lik.log_Rchols, horizon, x0s=x0s, **kw)
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        starts = [self._X_chains[s_][-1] for s_ in range(S)] if x0s is None else list(x0s)
        return explicit(Lm, lay.Z, lay.kernel, [lay.U] * S, None, starts, ci, n_train, Y_test, self.Q, lik.CC, lik.DD, lik.log_Rchols,
                        horizon, **kw)

    FORECAST_SCORE_METHODS = ("moment", "linearised", "cubature", "particle", "adapted")

    def forecast_scores(self, Y_test, control_inputs=None, horizon=10, *, method="moment", levels=(0.05, 0.5, 0.95), use="auto", **kwargs):
        """CRPS, PIT, coverage and predictive quantiles of the k-step-ahead forecasts of a held-out record, k = 1 .. horizon: the
        prediction-level call of `forecast_heldout` (method "moment"), `forecast_heldout_linearised`, `forecast_heldout_cubature`,
        `forecast_heldout_particle` or `forecast_heldout_adapted` with its tracks (and, for the two particle rules, its particles)
        returned, then prediction.forecast_score on that fan.  kwargs: the keywords of that method's `forecast_heldout_*` except
        return_tracks (stride, origins, x0, S0, q_mode, Y_train_std; num_particles, seed, noise for the particle rules).  The three
        Gaussian rules are scored as the mixture of the chains' Gaussians; the particle rules by `use`: "auto" / "particles" the
        mixture of all S N particles' emissions, "moments" the per-chain Gaussians (m_fc, S_fc).  For "adapted" fc_particles is the
        set after the draw: its point mixture is the sampled form of the Rao-Blackwellised predictive that rule's ll_h reports.
        Returns the dict of prediction.forecast_score (crps, pit (B, horizon, Ydim), quantiles (B, horizon, Ydim, Q), crps_h,
        coverage_h, n_h, ...) plus the forecast's own dict under "fan"."""
        from . import prediction as pr
        who = "forecast_scores"
        if method not in DGPSSM.FORECAST_SCORE_METHODS:
            raise ValueError(f"{who}: method: expected one of {list(DGPSSM.FORECAST_SCORE_METHODS)}, got {method!r}")
        if use not in pr.SCORE_USES:
            raise ValueError(f"{who}: use: expected one of {list(pr.SCORE_USES)}, got {use!r}")
        particles = method in ("particle", "adapted")
        if use == "particles" and not particles:
            raise ValueError(f"{who}: use=\"particles\" needs a particle rule (method \"particle\" or \"adapted\"), got {method!r}")
        allowed = dict(stride=1, origins=None, x0=None, S0=None, q_mode="reference", Y_train_std=1.0)
        if particles:
            allowed.update(num_particles=256, seed=None, noise="shared")
        unknown = sorted(set(kwargs) - set(allowed))
        if unknown:
            raise TypeError(f"{who}: method {method!r} takes the keywords {sorted(allowed)}, got {unknown}")
        k = dict(allowed, **kwargs)
        pr._pack_levels(who, levels)                                # before any device work
        if particles:
            fan = DGPSSM._forecast_heldout_particles(self, who, method == "adapted", Y_test, control_inputs, horizon, k["num_particles"],
                                                     k["seed"], k["noise"], k["stride"], k["origins"], k["x0"], k["S0"], k["q_mode"],
                                                     k["Y_train_std"], True, return_particles=use != "moments")
        else:
            fan = DGPSSM._forecast_heldout(self, who, method, Y_test, control_inputs, horizon, k["stride"], k["origins"], k["x0"], k["S0"],
                                           k["q_mode"], k["Y_train_std"], True)
        lik = self.likelihood
        Y = np.asarray(Y_test, dtype=np.float64)
        res = pr.forecast_score(fan, Y, lik.CC, lik.DD, lik.log_Rchols, levels=levels, use=use, Y_train_std=k["Y_train_std"])
        res["fan"] = fan
        return res

    def predict_transition(self, Xnew, *, q_mode="reference", per_chain=True):
        """The learned transition function at inputs of the caller's choice: mean and variance of the posterior GP increment
        f(x, c) at the rows of Xnew (N, D + C) -- the f_mu and f_var a rollout adds at every step (x_next = x + f_mu +
        eps sqrt(f_var + Q), base_model.py:304-314).  This is f itself: NOT x_next (add x, and Q to the variance, for that) and
        NOT y (the emission C x + d with its noise is not applied).
        Collapsed U: the S = num_chains posteriors U | X_s in one fused `posterior_conditional_grouped` call (G = S, one model);
        q_mode "reference" inflates every dim with slice 0 of L_H^-T as the reference and the rollouts do, "intent"
        dim d with slice d.  Explicit U: f does not depend on the chain, so one group is evaluated (no q_sqrt term) and `mean` /
        `var` have a leading axis of 1.  Parameters newer on the device than on the host are pulled first.
        Returns a dict: mean, var (S or 1, N, D; None unless per_chain), mix_mean, mix_var (N, D): the equal-weight mixture over
        the chains."""
        from . import conditionals_multi_output as cmo
        from .prediction import posterior_conditional_grouped
        if q_mode not in cmo.Q_MODES:
            raise ValueError(f"predict_transition: q_mode: expected one of {sorted(cmo.Q_MODES)}, got {q_mode!r}")
        if self._host_stale:
            self.pull_parameters()
        lay = self.layers[-1]
        if self.U_collapse:
            S = self.num_chains
            mean, var, mm, mv = posterior_conditional_grouped(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q,
                                                              self.control_inputs, Xnew, q_mode=q_mode, per_group=bool(per_chain))
        else:
            Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
            mean, var, mm, mv = cmo.conditional_grouped(Lm, lay.Z, lay.kernel, [lay.U], None, Xnew, q_mode=q_mode,
                                                        per_group=bool(per_chain))
        return dict(mean=mean, var=var, mix_mean=mm, mix_var=mv)

    def linearize(self, Xnew, *, q_mode="reference", per_chain=True):
        """The local linear model of the learned transition at the rows of Xnew (N, D + C): `predict_transition` together with the
        gradients of mean and variance of f(x, c) with respect to x and c, in closed form (SE-ARD kernels only).
        A = I + d mean / dx and B = d mean / dc: A is the Jacobian of x + f(x, c), i.e. of the TRANSITION MEAN x_next = x + f_mu, not
        of f (subtract I for that); B is the same for both.  x_next ~= x_next(x0, c0) + A (x - x0) + B (c - c0) is what an EKF,
        iLQR / MPC or a stability analysis takes; dvar is the gradient of the predictive variance of f (the process noise Q does not
        depend on the input).
        Collapsed U: the S = num_chains posteriors in one fused `posterior_conditional_grad_grouped` call; explicit U: one group
        (leading axis 1), no q_sqrt term -- the split and q_mode of `predict_transition`.
        Returns a dict: mean, var (S or 1, N, D), dmean, dvar (S or 1, N, D, D + C), A (S or 1, N, D, D), B (S or 1, N, D, C) (None
        unless per_chain); mix_mean, mix_var (N, D), mix_dmean, mix_dvar (N, D, D + C), mix_A (N, D, D), mix_B (N, D, C): the
        equal-weight mixture over the chains, mix_A = I + mix_dmean[..., :D]."""
        from . import conditionals_multi_output as cmo
        from .prediction import posterior_conditional_grad_grouped
        if q_mode not in cmo.Q_MODES:
            raise ValueError(f"linearize: q_mode: expected one of {sorted(cmo.Q_MODES)}, got {q_mode!r}")
        if self._host_stale:
            self.pull_parameters()
        lay = self.layers[-1]
        if self.U_collapse:
            S = self.num_chains
            out = posterior_conditional_grad_grouped(lay.Z, lay.kernel, [self._X_chains[s_] for s_ in range(S)], self.Q,
                                                     self.control_inputs, Xnew, q_mode=q_mode, per_group=bool(per_chain))
        else:
            Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
            out = cmo.conditional_grad_grouped(Lm, lay.Z, lay.kernel, [lay.U], None, Xnew, q_mode=q_mode, per_group=bool(per_chain))
        for key, a_key, b_key in (("dmean", "A", "B"), ("mix_dmean", "mix_A", "mix_B")):
            dm = out[key]
            D = None if dm is None else dm.shape[-2]
            out[a_key] = None if dm is None else np.eye(D) + dm[..., :D]
            out[b_key] = None if dm is None else np.ascontiguousarray(dm[..., D:])
        return out
