"""The ``+backbone=sindy`` plugin on MI355X: drop-in for the reference ``SINDY`` model
(``libs_m/ct/src/models/sindy.py:57-431, 717-760``; metrics inherited from
``libs_m/ct/src/models/time_varying_model.py:236-313``).

Same constructor (``SINDY(args, dataset_collection)``), methods (``fit``, ``get_predictions``,
``get_autoregressive_predictions``, ``get_normalised_masked_rmse``,
``get_normalised_n_step_rmses``), attributes (``global_equation_string``, ``joint_coefs``,
``feature_library_names``, ``insite``, ``hparams``) and error behaviour (Python exceptions;
``AssertionError`` on NaN predictions).  The two inner call sites of the reference run on the GPU
through the C ABI (include/insite_hip.h):

* ``SINDy(...).fit(X_a, u=U_a, t=dt, multiple_trajectories=True)`` per arm (sindy.py:190-192)
  -> ``insite_sindy_fit_f64``: smoothing + 4th-order FD + library + per-arm Gram in one streaming
  kernel, then the reduction fused with STLSQ + unbias for every arm.
* ``jit(vmap(simulate_cancer_volume))`` (sindy.py:413-431) -> ``insite_rollout_f64`` (Euler-5).
* ``insite: true`` — ``pmap(vmap(simulate_cancer_volume_with_fine_tuning))`` (sindy.py:433-715): the
  per-patient BFGS refinement -> ``insite_refine_f64`` (one lane per patient; 4-arm datasets:
  ``insite_refine_arms_f64``).

The DE-format extraction (A1, pkpd/utils.py:523-606), the tau-step slice (A9) and the masked
squared-error sums of the metrics (A10) also run on the device; only scalars and the returned
prediction arrays cross back to the host.  The cancer_sim / EQ_5 datasets run the
treatment-segment discovery (``insite_sindy_fit_segments_f64``), the 4-arm rollout and, with
``insite: true``, the 4-arm refinement.  The ablations run through the general one-state path
(``insite_gen_gram_f64``): ``ablation_more_complex_basis_functions`` (PolynomialLibrary(degree=4,
interaction_only=False), sindy.py:185-186; EQ_4) and ``joint_model`` (one regression with the multilabel
treatment(s) as library inputs, pkpd/utils.py:486-497, 639-672; sindy.py:283-288, 313-322), whose RHS
is folded per treatment combination into the per-arm rollout; with ``insite: true`` both refine on the
GPU (``insite_refine_general_f64``: the joint model's coefficients act on the treatment combinations their
inputs switch on; the degree-4 library runs the state-polynomial refinement kernels).  The degree-4 library
on the treatment-segment datasets runs ``insite_gen_gram_segments_f64`` (per-arm power moments of the
segment rows).  Weak SINDy (the reference's ``wsindy`` backbone: WeakPDELibrary(K=100) + SR3) runs through the
model key ``weak_form`` (``fit_weak``: ``insite_sindy_fit_weak_f64``); the key ``wsindy: true``
itself still raises ``NotImplementedError``.  ``bootstrap`` / ``bootstrap_irregular`` refit the per-arm model on
patient-level Poisson resamples from the per-patient moments (``insite_sindy_bootstrap_f64``) and
``predict_interval`` turns the replicates into pointwise prediction bands.  ``predict_bands`` and
``treatment_effect`` give the bands of every row, and of the paired effect of two treatment plans, without
materialising the replicate trajectories (``insite_effect_bands_f64``).  On the treatment-segment
datasets ``bootstrap_segments`` draws the ensemble (one weight per patient for all of their segments,
``insite_segboot_fit_f64``) and opens the same methods.
"""
from __future__ import annotations

import logging

import numpy as np
import torch

from . import _lib, bootstrap, effect, ops, weak
from .library import polynomial_library

logger = logging.getLogger(__name__)

MAX_SEQUENCE_LENGTH = 60
MAX_TIME_HORIZON = 10.0
STANDARD_DT = MAX_TIME_HORIZON / MAX_SEQUENCE_LENGTH   # pkpd/utils.py:53; SINDY.dt (sindy.py:89)
RHS_COEF_EPS = 1e-3                                    # pkpd/utils.py:388


# scipy.signal.savgol_filter(window_length=5, polyorder=3, mode='interp') weights: interior taps and the
# polynomial-fit edge rows (the same table as the HIP kernels' sg_pos*/sg_interior)
_SG53 = np.array([[69, 4, -6, 4, -1], [4, 54, 24, -16, 4], [-3, 12, 17, 12, -3], [4, -16, 24, 54, 4],
                  [-1, 4, -6, 4, 69]], dtype=np.float64) / np.array([70, 70, 35, 70, 70], dtype=np.float64)[:, None]


def savgol_5_3_rows(V: torch.Tensor) -> torch.Tensor:
    """savgol(5, 3, mode='interp') along the time axis of [N, T] device rows (T >= 5)."""
    W = torch.as_tensor(_SG53, device=V.device, dtype=V.dtype)
    T = V.size(1)
    out = torch.empty_like(V)
    c = W[2]
    out[:, 2:T - 2] = (c[0] * V[:, 0:T - 4] + c[1] * V[:, 1:T - 3] + c[2] * V[:, 2:T - 2] + c[3] * V[:, 3:T - 1]
                       + c[4] * V[:, 4:T])
    out[:, :2] = V[:, :5] @ W[:2].t()
    out[:, T - 2:] = V[:, T - 5:] @ W[3:].t()
    return out


def _get(cfg, path, default=None):
    """Read ``a.b.c`` from a nested dict / attribute config (DictConfig-like)."""
    cur = cfg
    for key in path.split("."):
        if cur is None:
            return default
        if isinstance(cur, dict):
            cur = cur.get(key, None)
        else:
            cur = getattr(cur, key, None)
    return default if cur is None else cur


def equation_terms(coefs, names, quantize=False, round_to=3) -> str:
    """Term string of ``convert_sindy_model_to_sympyjax_model_core`` (pkpd/utils.py:378-397):
    ``+{c}*term`` for every |c| > 1e-3, with numpy's shortest round-trip float formatting."""
    s = ""
    for j, c in enumerate(np.asarray(coefs, dtype=np.float64)):
        if np.abs(c) > RHS_COEF_EPS:
            if quantize:
                c = np.round(c, round_to)
            s += f"+{c}*" + names[j].replace(" ", "*")
    return s


def equation_string(joint_coefs, names, quantize=False, round_to=3) -> str:
    """``global_equation_string`` (sindy.py:276): 'Treatment 0: x_dot = ... | Treatment 1: ...'."""
    return " | ".join(f"Treatment {a}: x_dot = {equation_terms(c, names, quantize, round_to)}"
                      for a, c in enumerate(np.asarray(joint_coefs)))


def rhs_coefficients(joint_coefs, quantize=False, round_to=3) -> np.ndarray:
    """Coefficient table the sympy RHS evaluates: terms with |c| <= 1e-3 dropped, optionally
    rounded (the rounded value is what ``sympify`` of the string parses back)."""
    c = np.asarray(joint_coefs, dtype=np.float64).copy()
    keep = np.abs(c) > RHS_COEF_EPS
    if quantize:
        c = np.round(c, round_to)
    return np.where(keep, c, 0.0)


class SINDY:
    """MI355X drop-in for ``src.models.sindy.SINDY`` (EQ_4 PK/PD datasets, non-joint model)."""

    model_type = "sindy_regressor"
    tuning_criterion = "rmse"

    def __init__(self, args, dataset_collection=None, autoregressive=None, has_vitals=None, device=None, **kwargs):
        self.hparams = args
        self.dataset_collection = dataset_collection
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()
                                                                                    if torch.cuda.is_available() else 0)
        m = lambda k, d=None: _get(args, f"model.{k}", d)   # noqa: E731
        self.lag_features = m("lag_features", 1)
        self.dim_outcome = int(m("dim_outcomes", 1))
        self.dim_treatments = int(m("dim_treatments", 2))
        self.dim_static_features = int(m("dim_static_features", 2))
        self.dim_vitals = int(m("dim_vitals", 0))
        self.smoother_kws = {"window_length": 5, "polyorder": 3}
        self.dt = float(m("dt", STANDARD_DT))   # reference hard-codes STANDARD_DT
        self.insite_val_error_threshold = m("insite_val_error_threshold")
        self.global_equation_string = ""
        self.sindy_threshold = float(m("sindy_threshold"))
        self.sindy_alpha = float(m("sindy_alpha"))
        self.smooth_input_data = bool(m("smooth_input_data", False))
        self.sindy_quantize = bool(m("sindy_quantize", False))
        self.sindy_quantize_global_model_round_to = int(m("sindy_quantize_global_model_round_to", 2))
        self.lam = m("lam")
        self.joint_model = bool(m("joint_model", False))
        self.insite = bool(m("insite", False))
        self.wsindy = bool(m("wsindy", False))
        self.weak_form = bool(m("weak_form", False))    # the reference's wsindy backbone on the GPU (fit_weak)
        self.weak_K = int(m("weak_K", weak.DEFAULT_K))
        self.weak_p = int(m("weak_p", weak.DEFAULT_P))
        self.weak_seed = m("weak_seed")
        self.weak_optimizer = str(m("weak_optimizer", "sr3"))
        self.use_smoothed_finite_difference = bool(m("use_smoothed_finite_difference", False))
        self.dataset_name = str(m("dataset_name", ""))
        # cancer_sim / EQ_5: treatment-segment split, FiniteDifference(order=1), one fit per arm of
        # the 4-valued treatment (sindy.py:160-183, 193-216, 289-312)
        self.segment_mode = "EQ_5" in self.dataset_name.upper() or "CANCER_SIM" in self.dataset_name.upper()
        self.ablation_more_complex_basis_functions = bool(m("ablation_more_complex_basis_functions", False))
        self.insight_recover_parametric_dist = bool(m("insight_recover_parametric_dist", False))
        self.treatment_mode = _get(args, "dataset.treatment_mode", "multiclass")
        self.projection_horizon = int(_get(args, "dataset.projection_horizon", 5))
        self.unscale_rmse = bool(_get(args, "exp.unscale_rmse", True))
        self.percentage_rmse = bool(_get(args, "exp.percentage_rmse", True))
        self.integrator = str(m("integrator", "euler5"))   # reference: Euler-5 (pkpd/utils.py:68-94)
        # BFGS status 3 -> global model (the code at sindy.py:628-631) or keep the iterate (the published
        # runs): default follows the published outputs
        self.insite_revert_on_zoom_fail = bool(m("insite_revert_on_zoom_fail", False))
        # PolynomialLibrary(**PolynomialLibrary_kw) of sindy.py:185-188
        self.lib_degree, self.lib_interaction_only = (4, False) if self.ablation_more_complex_basis_functions else (2, True)
        self.library = polynomial_library(self.dim_static_features, self.lib_degree, self.lib_interaction_only)
        self.feature_library_names = self.library.get_feature_names()
        self._roll_library = self.library   # the library the rollout evaluates (joint: folded per combination)
        self.feature_names = ["x0"] + [f"u{i}" for i in range(self.dim_static_features)]
        self.joint_coefs = None
        self.n_iter = None
        self._coef_dev = None
        self._check_supported()

    # ------------------------------------------------------------------ configuration checks
    def _check_supported(self):
        if not (self.segment_mode or "EQ_4" in self.dataset_name.upper()):
            raise NotImplementedError(f"dataset {self.dataset_name!r}: this build covers the PK/PD EQ_4 family and "
                                      "the treatment-segment datasets (cancer_sim, EQ_5_*)")
        if self.wsindy:
            raise NotImplementedError("weak SINDy (wsindy: true) is not on the MI355X path; "
                                      "the GPU weak form is model.weak_form (+backbone=weak)")
        if self.weak_optimizer not in ops.WEAK_OPTIMIZERS:
            raise ValueError(f"weak_optimizer must be one of {sorted(ops.WEAK_OPTIMIZERS)}")
        if self.integrator not in ops.METHODS:
            raise ValueError(f"integrator must be one of {sorted(ops.METHODS)}")

    def prepare_data(self) -> None:
        c = self.dataset_collection
        if c is not None and not getattr(c, "processed_data_multi", True):
            c.process_data_multi()

    # ------------------------------------------------------------------ A1: DE format on device
    def _unscaled_inputs(self, dataset):
        sp = dataset.scaling_params
        d = dataset.data
        dev = self.device
        std, mean = float(sp["output_stds"]), float(sp["output_means"])
        prev = torch.as_tensor(np.ascontiguousarray(d["prev_outputs"][..., 0]), device=dev) * std + mean
        lo, hi = self.dim_outcome, self.dim_outcome + self.dim_static_features
        stat = (torch.as_tensor(np.ascontiguousarray(d["static_features"]), device=dev)
                * torch.as_tensor(np.asarray(sp["inputs_stds"][lo:hi], dtype=np.float64), device=dev)
                + torch.as_tensor(np.asarray(sp["input_means"][lo:hi], dtype=np.float64), device=dev))
        return prev, stat.contiguous(), std, mean

    def de_format(self, dataset, sequence_lengths_offset=1):
        """Device arrays of ``process_dataset_into_de_format`` (pkpd/utils.py:523-606): the
        reconstructed volume series x[N,T] (prev_outputs[:,0] ++ unscaled_outputs), statics u[N,U],
        the arm of each patient (current_treatments[:,0] == [1,0] -> 0, else 1; utils.py:425) and
        the discovery rows seq_len - offset (utils.py:426).  ``smooth_input_data`` smooths a copy
        the reference never reads back (utils.py:568-571), so it has no effect there or here."""
        d = dataset.data
        prev, stat, _, _ = self._unscaled_inputs(dataset)
        uo = torch.as_tensor(np.ascontiguousarray(d["unscaled_outputs"][..., 0]), device=self.device)
        x = torch.cat([prev[:, :1], uo], dim=1).contiguous()
        ct = torch.as_tensor(np.ascontiguousarray(d["current_treatments"][:, 0, :]), device=self.device)
        arm = torch.where((ct[:, 0] == 1) & (ct[:, 1] == 0), 0, 1).to(torch.int8)
        rows = (torch.as_tensor(np.asarray(d["sequence_lengths"]), device=self.device).to(torch.int64)
                - sequence_lengths_offset).to(torch.int32)
        return x, stat, arm, rows

    def de_format_segments(self, dataset):
        """Device arrays of the cancer_sim / EQ_5 branch of ``process_dataset_into_de_format``
        (pkpd/utils.py:607-637, sequence_lengths_offset = 0): the reconstructed series x[N, T], statics
        u[N, U], the per-step arm argmax(current_treatments) [N, T-1] (utils.py:624) and seq_len[N].
        The treatment-constant segments themselves are cut inside the Gram kernel."""
        d = dataset.data
        prev, stat, _, _ = self._unscaled_inputs(dataset)
        uo = torch.as_tensor(np.ascontiguousarray(d["unscaled_outputs"][..., 0]), device=self.device)
        x = torch.cat([prev[:, :1], uo], dim=1).contiguous()
        arm = torch.as_tensor(np.argmax(d["current_treatments"], axis=-1).astype(np.int8), device=self.device)
        sl = torch.as_tensor(np.asarray(d["sequence_lengths"]).astype(np.int32), device=self.device)
        return x, stat, arm.contiguous(), sl

    def _fit_segments(self, train_f):
        """cancer_sim / EQ_5 discovery (sindy.py:160-216): segment split + FD order 1 (or the
        savgol(2, 1)-smoothed variant) + library + per-arm Gram in one kernel, STLSQ per arm fused into
        the reduction launch (insite_sindy_fit_segments_f64)."""
        x, u, arm, sl = self.de_format_segments(train_f)
        fd = "smoothed1" if self.use_smoothed_finite_difference else "order1"
        if self.library.state_degree > 1:   # the degree-4 ablation library: per-arm power moments (insite_gen.hip)
            G, b = ops.gen_gram_segments(x, arm, sl, u, self.dt, self.library, n_arms=self.dim_treatments, fd=fd)
            coef, mask, iters = ops.stlsq(G, b, self.sindy_threshold, self.sindy_alpha, 100, True)
            return coef, mask, iters, G, b
        return ops.sindy_fit_segments(x, arm, sl, u, self.dt, self.library, self.sindy_threshold, self.sindy_alpha,
                                      max_iter=100, unbias=True, n_arms=self.dim_treatments, fd=fd)

    # ------------------------------------------------------------------ discovery
    def _fit_joint(self, train_f):
        """The joint ("one ODE") model (sindy.py:190, 203 with joint_model; DE format pkpd/utils.py:639-672):
        ONE regression over the rows x = unscaled_outputs[:seq_len - offset] (offset 1 for EQ_4, 0 for
        cancer_sim / EQ_5) with library inputs (x0, treatment bits, statics) — the multilabel treatments of
        ``dataset.treatment_mode=multilabel`` (run.py:198-201).  General one-state Gram + STLSQ on the GPU."""
        d = train_f.data
        ct = np.asarray(d["current_treatments"])
        if ct.ndim != 3 or ct.shape[-1] > 2 or not np.all((ct == 0) | (ct == 1)):
            raise NotImplementedError("joint_model needs binary multilabel treatments (dataset.treatment_mode="
                                      "multilabel, at most 2 treatment columns)")
        n_in = ct.shape[-1]
        self.library = polynomial_library(self.dim_static_features, self.lib_degree, self.lib_interaction_only,
                                          n_inputs=n_in)
        self.feature_library_names = self.library.get_feature_names()
        self.feature_names = list(self.library.input_names)
        _, stat, _, _ = self._unscaled_inputs(train_f)
        x = torch.as_tensor(np.ascontiguousarray(d["unscaled_outputs"][..., 0]), device=self.device)
        code = torch.as_tensor(self._treatment_code(ct), device=self.device)
        offset = 0 if self.segment_mode else 1
        rows = (torch.as_tensor(np.asarray(d["sequence_lengths"]), device=self.device).to(torch.int64) - offset)
        if self.segment_mode:
            fd, need = ("smoothed1" if self.use_smoothed_finite_difference else "order1"), 2
        else:
            fd, need = "smoothed4", 5
        if int(rows.min().item()) < need:
            raise ValueError(f"a training trajectory has fewer than {need} rows for the {fd} derivative")
        coef, mask, iters, _, _ = ops.gen_sindy_fit(x, stat, rows.to(torch.int32), self.dt, self.library,
                                                    self.sindy_threshold, self.sindy_alpha, step_in=code, fd=fd)
        return self._finish_fit(coef, mask, iters)

    @staticmethod
    def _treatment_code(ct) -> np.ndarray:
        """Per-step input code of binary multilabel treatments [N, T, n_in]: bit i = treatment i."""
        ct = np.asarray(ct)
        code = np.zeros(ct.shape[:2], dtype=np.int8)
        for i in range(ct.shape[-1]):
            code |= (ct[..., i].astype(np.int8) << i)
        return np.ascontiguousarray(code)

    def _fold_joint(self, rhs):
        """The joint RHS sum_j c_j x^e_j in(k)^tau_j m_j(u) as per-combination (arm) coefficients over the
        library with the input columns dropped: combination c keeps the columns whose inputs are all on in
        c (binary inputs), so the per-arm rollout kernels evaluate the same f(y, in_k, u)."""
        lib = self.library
        n_in, U = lib.n_inputs, lib.n_statics
        e = lib.exps
        keep_cols = [0] + list(range(1 + n_in, 1 + n_in + U))
        red_rows, index = [], []
        for row in e[:, keep_cols].tolist():
            if row not in red_rows:
                red_rows.append(row)
            index.append(red_rows.index(row))
        from .library import PolyLibrary
        red = PolyLibrary(np.array(red_rows, dtype=np.int8), (lib.input_names[0],) + tuple(lib.input_names[1 + n_in:]))
        NC = 1 << n_in
        folded = np.zeros((NC, len(red_rows)))
        tin = [(sum(1 << i for i in range(n_in) if e[j, 1 + i] > 0)) for j in range(lib.n_terms)]
        for c in range(NC):
            for j in range(lib.n_terms):
                if (tin[j] & ~c) == 0:
                    folded[c, index[j]] += rhs[0, j]
        return red, folded

    def fit(self, train_f, val_f=None):
        """Global discovery per arm (sindy.py:145-336): one Gram pass + STLSQ on the GPU."""
        self.prepare_data()
        if self.weak_form:
            return self.fit_weak(train_f, K=self.weak_K, p=self.weak_p, seed=self.weak_seed,
                                 optimizer=self.weak_optimizer)
        if self.joint_model:
            return self._fit_joint(train_f)
        if self.segment_mode:
            coef, mask, iters, G, _ = self._fit_segments(train_f)
            empty = np.nonzero(G[:, 0, 0].cpu().numpy() == 0)[0]
            if empty.size:
                raise ValueError(f"treatment arm(s) {empty.tolist()} have no training segments "
                                 "(pysindy cannot fit an empty trajectory list)")
            return self._finish_fit(coef, mask, iters)
        x, u, arm, rows = self.de_format(train_f)
        if int(rows.min().item()) < 5:
            raise ValueError("a training trajectory has fewer than 5 rows: the savgol(5, 3) smoother "
                             "and the 5-point derivative need at least 5 samples")
        if self.library.state_degree > 1:     # the degree-4 ablation library: the general path
            coef, mask, iters, _, _ = ops.gen_sindy_fit(x, u, rows, self.dt, self.library, self.sindy_threshold,
                                                        self.sindy_alpha, group=arm, n_groups=self.dim_treatments,
                                                        fd="smoothed4")
            return self._finish_fit(coef, mask, iters)
        coef, mask, iters, _, _ = ops.sindy_fit(x, u, arm, rows, self.dt, self.library, self.sindy_threshold,
                                                self.sindy_alpha, max_iter=100, unbias=True,
                                                n_arms=self.dim_treatments, fd="smoothed4")
        return self._finish_fit(coef, mask, iters)

    def _finish_fit(self, coef, mask, iters):
        iters_h = iters.cpu().numpy()
        if np.any(iters_h < 0):
            raise np.linalg.LinAlgError("STLSQ / SR3 system is not positive definite")
        self.joint_coefs = coef.cpu().numpy()
        self.coef_mask = mask.cpu().numpy().astype(bool)
        self.n_iter = iters_h
        rhs = rhs_coefficients(self.joint_coefs, self.sindy_quantize, self.sindy_quantize_global_model_round_to)
        if self.joint_model:
            self._roll_library, rhs = self._fold_joint(rhs)
            self.global_equation_string = "Joint Model: x_dot = " + equation_terms(
                self.joint_coefs[0], self.feature_library_names, self.sindy_quantize,
                self.sindy_quantize_global_model_round_to)                           # sindy.py:285, 315
        else:
            self._roll_library = self.library
            self.global_equation_string = equation_string(self.joint_coefs, self.feature_library_names,
                                                          self.sindy_quantize, self.sindy_quantize_global_model_round_to)
        self._coef_dev = torch.as_tensor(np.ascontiguousarray(rhs), device=self.device)
        logger.info("[Model]: %s", self.global_equation_string)
        return self

    # ------------------------------------------------------------------ weak form (the reference's wsindy backbone)
    def fit_weak(self, train_f, K=weak.DEFAULT_K, p=weak.DEFAULT_P, H=None, seed=None, optimizer="sr3"):
        """Weak-form discovery per arm (sindy.py:218-239: WeakPDELibrary(K) + SR3(l1, normalize_columns)) in one
        Gram pass + per-arm solve on the GPU (insite_sindy_fit_weak_f64).  The grid is the reference's
        t_train = arange(T) dt with T = the training rows (seq_len - 1); K subdomains with centres
        ``weak.draw_centres(T, dt, K, seed)``, half-width ``H`` (default L / 20) and exponent ``p``.  ``optimizer``:
        "sr3" (threshold = sindy_threshold, nu = 1, tol = 1e-1, max_iter = 1000) or "stlsq" (sindy_threshold,
        sindy_alpha).  Sets what ``fit`` sets."""
        if self.joint_model or self.segment_mode or self.library.state_degree > 1:
            raise NotImplementedError("fit_weak covers the per-arm EQ_4 model over the affine library")
        self.prepare_data()
        x, u, arm, rows = self.de_format(train_f)
        T = int(rows.max().item())
        if T < 2:
            raise ValueError("the weak form needs trajectories of at least 2 rows")
        # sorted: the sum over the subdomains does not depend on their order, and the kernel skips the all-zero
        # tiles of 16 consecutive rows of W | D
        centres = np.sort(weak.draw_centres(T, self.dt, K, seed, H=H))
        W, D = weak.test_function_weights(T, self.dt, centres, H=H, p=p, device=self.device)
        xs = x[:, :T]
        coef, mask, iters, G, _ = ops.sindy_fit_weak(xs, W, D, u, arm, rows, self.library, self.sindy_threshold,
                                                     optimizer=optimizer, alpha=self.sindy_alpha,
                                                     n_arms=self.dim_treatments)
        empty = np.nonzero(G[:, 0, 0].cpu().numpy() == 0)[0]
        if empty.size:
            raise ValueError(f"treatment arm(s) {empty.tolist()} have no trajectory of {T} rows "
                             "(pysindy cannot fit an empty trajectory list)")
        return self._finish_fit(coef, mask, iters)

    # ------------------------------------------------------------------ irregular observation grids (C5)
    def fit_irregular(self, x, t_obs, n_obs, u, arm, fd="nonuniform4", validate=True):
        """Global discovery per arm from trajectories sampled at each patient's own times
        (insite_sindy_fit_irregular_f64): device tensors x, t_obs [N, T_max] patient-major, n_obs [N] int32,
        u [N, U], arm [N] int8 (one factual arm per patient).  ``fd``: "nonuniform2" or "nonuniform4" (the
        Lagrange derivative through 3 / 5 samples; pysindy FiniteDifference(order=2, is_uniform=False) and its
        five-point form).  Sets ``joint_coefs``, ``global_equation_string`` and the rollout model as ``fit``."""
        if self.joint_model or self.segment_mode or self.library.state_degree > 1:
            raise NotImplementedError("fit_irregular covers the per-arm EQ_4 model over the affine library")
        coef, mask, iters, G, _ = ops.sindy_fit_irregular(x, t_obs, n_obs, u, arm, self.library, self.sindy_threshold,
                                                          self.sindy_alpha, max_iter=100, unbias=True,
                                                          n_arms=self.dim_treatments, fd=fd, validate=validate)
        empty = np.nonzero(G[:, 0, 0].cpu().numpy() == 0)[0]
        if empty.size:
            raise ValueError(f"treatment arm(s) {empty.tolist()} have no trajectory long enough for {fd} "
                             "(pysindy cannot fit an empty trajectory list)")
        return self._finish_fit(coef, mask, iters)

    def predict_irregular(self, y0, u, arm_bits, t_obs, n_obs, **kwargs):
        """Adaptive RK45 rollout of the fitted model on per-patient grids: ``ops.rollout_rk45`` with the fitted
        coefficients (its arguments and layouts; returns (y, step attempts))."""
        if self._coef_dev is None:
            raise RuntimeError("fit() first")
        return ops.rollout_rk45(y0, u, arm_bits, t_obs, n_obs, self._coef_dev, self._roll_library, **kwargs)

    # ------------------------------------------------------------------ patient-level bootstrap
    IRREGULAR_WINDOW = {"nonuniform2": 3, "nonuniform4": 5}   # samples the Lagrange derivative needs

    def _check_bootstrap(self, what, resample=False):
        """``resample``: ``what`` draws an ensemble of the one-arm-per-patient model itself (``bootstrap``,
        ``bootstrap_irregular``).  Every other caller consumes ``bootstrap_``; a treatment-segment model may, once
        ``bootstrap_segments`` has stored its own ensemble (``bootstrap_mode_ == "segments"``)."""
        if self.joint_model or self.library.state_degree > 1:
            raise NotImplementedError(f"{what} covers the per-arm model over the affine library (not the joint or "
                                      "degree-4 modes)")
        if self.segment_mode and (resample or getattr(self, "bootstrap_mode_", None) != "segments"):
            raise NotImplementedError(f"{what}: a treatment-segment model (cancer_sim, EQ_5_*) takes its ensemble "
                                      "from bootstrap_segments()")

    def _bootstrap_moments(self, mom, u, arm, rows, min_rows, n_replicates, seed, quantiles, optimizer, max_iter):
        """The replicates' fits from per-patient moments with the model's own solver parameters -> bootstrap_."""
        coef, mask, iters, _, _ = ops.sindy_bootstrap(mom, u, arm, rows, self.library, n_replicates,
                                                      self.sindy_threshold, optimizer=optimizer,
                                                      alpha=self.sindy_alpha, max_iter=max_iter, unbias=True,
                                                      seed=seed, n_arms=self.dim_treatments, min_rows=min_rows)
        self.bootstrap_ = bootstrap.summarize(coef, mask, quantiles, seed=int(seed))
        self.bootstrap_iters_ = iters
        self.bootstrap_mode_ = "arms"
        return self.bootstrap_

    def bootstrap_segments(self, train_f, n_replicates=256, seed=0, quantiles=(0.025, 0.5, 0.975)):
        """``bootstrap`` for the treatment-segment datasets (cancer_sim, EQ_5_*; insite_segboot.h):
        ``n_replicates`` refits of the per-arm segment regression of ``fit``, each on the cohort with every patient
        -- all of its segments, in every arm -- weighted by one Poisson(1) count; replicate 0 has weight 1 everywhere
        (the fit itself).  Stores and returns ``self.bootstrap_`` and marks it as the segment model's own, which
        opens ``predict_interval``, ``predict_bands``, ``treatment_effect``, ``average_effect``,
        ``predict_average``, ``choose_plan``, ``policy_value``, ``evaluate_rules`` and ``rule_value`` to this model;
        the fitted model is not touched."""
        if not self.segment_mode:
            raise NotImplementedError("bootstrap_segments covers the treatment-segment datasets (cancer_sim, "
                                      "EQ_5_*); the EQ_4 family has bootstrap()")
        if self.weak_form or self.joint_model or self.library.state_degree > 1:
            raise NotImplementedError("bootstrap_segments covers the per-arm strong-form segment model over the "
                                      "affine library (not the weak_form, joint_model or degree-4 modes)")
        self.prepare_data()
        x, u, arm, sl = self.de_format_segments(train_f)
        fd = "smoothed1" if self.use_smoothed_finite_difference else "order1"
        mom = ops.segment_moments(x, arm, sl, self.dt, n_arms=self.dim_treatments, fd=fd)
        coef, mask, iters, _, _ = ops.sindy_bootstrap_segments(mom, u, self.library, n_replicates,
                                                               self.sindy_threshold, alpha=self.sindy_alpha,
                                                               max_iter=100, unbias=True, seed=seed)
        empty = np.nonzero(mom[:, :, 0].sum(0).cpu().numpy() == 0)[0]   # replicate 0's sample count per arm
        if empty.size:
            raise ValueError(f"treatment arm(s) {empty.tolist()} have no training segments "
                             "(pysindy cannot fit an empty trajectory list)")
        self.bootstrap_ = bootstrap.summarize(coef, mask, quantiles, seed=int(seed))
        self.bootstrap_iters_ = iters
        self.bootstrap_mode_ = "segments"
        return self.bootstrap_

    def bootstrap(self, train_f, n_replicates=256, seed=0, quantiles=(0.025, 0.5, 0.975)):
        """Patient-level Poisson bootstrap of the discovery (insite_sindy_bootstrap_f64): ``n_replicates`` refits of
        the model's own regression -- the strong form (``ops.gram_moments``' per-patient moments, STLSQ) or, under
        ``weak_form``, the weak form (the weak pass's moments, ``weak_optimizer``) -- each on the cohort with every
        patient weighted by a Poisson(1) count; replicate 0 has weight 1 everywhere (the fit itself).  Stores and
        returns ``self.bootstrap_`` (``bootstrap.BootstrapResult``); the fitted model is not touched.  Under
        ``weak_form`` the subdomain centres are drawn as ``fit`` draws them: they are the fitted model's only with a
        fixed ``weak_seed``."""
        self._check_bootstrap("bootstrap", resample=True)
        self.prepare_data()
        x, u, arm, rows = self.de_format(train_f)
        if self.weak_form:
            T = int(rows.max().item())
            if T < 2:
                raise ValueError("the weak form needs trajectories of at least 2 rows")
            centres = np.sort(weak.draw_centres(T, self.dt, self.weak_K, self.weak_seed))
            W, D = weak.test_function_weights(T, self.dt, centres, p=self.weak_p, device=self.device)
            mom = ops.gram_weak(x[:, :T], W, D, u, arm, rows, self.library, n_arms=self.dim_treatments,
                                moments=True)[2]
            return self._bootstrap_moments(mom, u, arm, rows, T, n_replicates, seed, quantiles, self.weak_optimizer,
                                           1000)
        if int(rows.min().item()) < 5:
            raise ValueError("a training trajectory has fewer than 5 rows: the savgol(5, 3) smoother "
                             "and the 5-point derivative need at least 5 samples")
        mom = ops.gram_moments(x, u, arm, rows, self.dt, self.library, n_arms=self.dim_treatments, fd="smoothed4")[5]
        return self._bootstrap_moments(mom, u, arm, rows, 5, n_replicates, seed, quantiles, "stlsq", 100)

    def bootstrap_irregular(self, x, t_obs, n_obs, u, arm, fd="nonuniform4", validate=True, n_replicates=256, seed=0,
                            quantiles=(0.025, 0.5, 0.975)):
        """``bootstrap`` on the irregular pass's per-patient moments (the arguments of ``fit_irregular``)."""
        self._check_bootstrap("bootstrap_irregular", resample=True)
        mom = ops.gram_irregular(x, t_obs, n_obs, u, arm, self.library, n_arms=self.dim_treatments, fd=fd,
                                 moments=True, validate=validate)[2]
        return self._bootstrap_moments(mom, u, arm, n_obs, self.IRREGULAR_WINDOW[fd], n_replicates, seed, quantiles,
                                       "stlsq", 100)

    def predict_interval(self, dataset, quantiles=(0.025, 0.975), max_rows=1024, return_replicates=False):
        """Pointwise prediction bands from ``bootstrap_``: the first ``max_rows`` rows of ``dataset`` are rolled out
        under every replicate's equations (one ``ops.rollout`` with per-row coefficients [n R, n_arms, F], the
        integrator and the coefficient clean-up of ``get_predictions``) and the quantiles are taken over the
        replicates 1..R-1.  Returns the standardised band [Q, n, T] (the scale of ``get_predictions``) and, with
        ``return_replicates``, the rollouts [n, R, T] as well (replicate 0: the point model)."""
        self._check_bootstrap("predict_interval")
        bs = getattr(self, "bootstrap_", None)
        if bs is None:
            raise RuntimeError("bootstrap() first")
        R = bs.n_replicates
        if R < 2:
            raise ValueError("predict_interval needs at least one resampled replicate (n_replicates >= 2)")
        d = dataset.data
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        n = prev.size(0) if max_rows is None else min(int(max_rows), prev.size(0))
        T = d["prev_outputs"].shape[1]
        arm = torch.as_tensor(np.argmax(d["current_treatments"][:n], axis=-1).astype(np.int8), device=self.device)
        coef = bs.coef.to(self.device)
        keep = coef.abs() > RHS_COEF_EPS                                   # rhs_coefficients, on the device
        if self.sindy_quantize:
            s = 10.0 ** self.sindy_quantize_global_model_round_to
            coef = torch.round(coef * s) / s
        coef = torch.where(keep, coef, torch.zeros_like(coef))
        A, F = coef.shape[1:]
        y = ops.rollout(prev[:n, 0].repeat_interleave(R).contiguous(), stat[:n].repeat_interleave(R, 0).contiguous(),
                        arm.repeat_interleave(R, 0).contiguous(), coef.repeat(n, 1, 1).contiguous(), self.library,
                        self.dt, method=self.integrator, drop_below=0.0, T=T)
        y = ((y - mean) / std).view(n, R, T)
        qt = torch.as_tensor([float(v) for v in quantiles], dtype=y.dtype, device=y.device)
        band = torch.quantile(y[:, 1:], qt, dim=1)
        return (band, y) if return_replicates else band

    # ------------------------------------------------------------------ effect bands
    def _effect_coef(self, what, cap=_lib.EFFECT_MAX_REPLICATES):
        """The replicates' coefficients [R, A, F] with ``predict_interval``'s clean-up (``rhs_coefficients``);
        ``cap``: the replicate cap of the kernel that ``what`` launches."""
        self._check_bootstrap(what)
        bs = getattr(self, "bootstrap_", None)
        if bs is None:
            raise RuntimeError("bootstrap() first")
        R = bs.n_replicates
        if not 2 <= R <= cap:
            raise ValueError(f"{what} needs 2 <= n_replicates <= {cap} "
                             f"(replicate 0 is the point model; {cap} is the kernel's cap), "
                             f"got {R}")
        coef = bs.coef.to(self.device)
        keep = coef.abs() > RHS_COEF_EPS
        if self.sindy_quantize:
            s = 10.0 ** self.sindy_quantize_global_model_round_to
            coef = torch.round(coef * s) / s
        return torch.where(keep, coef, torch.zeros_like(coef)).contiguous()

    def _plan_arms(self, dataset, plan, name):
        """A treatment plan as per-step arms int8 [N, T]: None (the dataset's own ``current_treatments``), an int
        (that arm at every step), an int array [N, T] or a one-hot array [N, T, A]."""
        ct = dataset.data["current_treatments"]
        N, T, A = ct.shape
        if plan is None:
            arm = np.argmax(ct, axis=-1)
        elif isinstance(plan, (int, np.integer)):
            arm = np.full((N, T), int(plan))
        else:
            arm = plan.detach().cpu().numpy() if isinstance(plan, torch.Tensor) else np.asarray(plan)
            if arm.shape == (N, T, A):
                arm = np.argmax(arm, axis=-1)
            elif arm.shape != (N, T) or not np.issubdtype(arm.dtype, np.integer):
                raise ValueError(f"{name}: expected None, an int, an int array [{N}, {T}] or a one-hot array "
                                 f"[{N}, {T}, {A}]")
        if arm.size and (arm.min() < 0 or arm.max() >= self.dim_treatments):
            raise ValueError(f"{name}: arms must lie in [0, {self.dim_treatments})")
        return torch.as_tensor(np.ascontiguousarray(arm.astype(np.int8)), device=self.device)

    def predict_bands(self, dataset, quantiles=(0.025, 0.975)):
        """``predict_interval`` for every row of ``dataset`` on its factual plan, from ``bootstrap_``: an
        ``effect.EffectResult`` with the one series "a" -- the point model's prediction, and mean, standard deviation
        and ``quantiles`` over the replicates 1..R-1 -- standardised like ``get_predictions``.  One launch of
        ``ops.effect_bands``: the [N, R, T] replicate rollouts never exist in memory."""
        coef = self._effect_coef("predict_bands")
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arm = self._plan_arms(dataset, None, "plan")
        out = ops.effect_bands(prev[:, 0].contiguous(), stat, arm, None, coef, self.library, self.dt, quantiles,
                               method=self.integrator, drop_below=0.0, T=arm.size(1))
        return effect.from_bands(out, quantiles, shift=mean, scale=std)

    def treatment_effect(self, dataset, plan_b, plan_a=None, quantiles=(0.025, 0.5, 0.975)):
        """The counterfactual trajectories of every row of ``dataset`` under ``plan_a`` and ``plan_b`` and their
        difference a - b, paired within each bootstrap replicate (the quantile of the differences is not the
        difference of the quantiles).  A plan is None (the dataset's own treatments), an int (that arm at every step),
        an int array [N, T] or a one-hot array [N, T, A].  Returns an ``effect.EffectResult`` with the series "a", "b"
        and "effect": a and b standardised like ``get_predictions``, the effect divided by the output's standard
        deviation only."""
        coef = self._effect_coef("treatment_effect")
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arm_a = self._plan_arms(dataset, plan_a, "plan_a")
        arm_b = self._plan_arms(dataset, plan_b, "plan_b")
        out = ops.effect_bands(prev[:, 0].contiguous(), stat, arm_a, arm_b, coef, self.library, self.dt, quantiles,
                               method=self.integrator, drop_below=0.0, T=arm_a.size(1))
        return effect.from_bands(out, quantiles, shift=mean, scale=std)

    # ------------------------------------------------------------------ scoring the bands
    def score_bands(self, dataset, levels=(0.5, 0.9, 0.95), n_bins=10, groups=None, plan=None):
        """How good the bands of ``bootstrap_`` are on a dataset with outcomes: per group (``groups`` as
        ``average_effect``'s) and step, and pooled over the steps, the coverage, width and interval score of the
        central bands of ``levels``, the rank (PIT) histogram with ``n_bins`` bins, the CRPS of the ensemble, its spread
        and the RMSE of the point model and of the ensemble mean -- an ``effect.EnsembleScore``, lengths standardised
        with the output's standard deviation.  Observations: ``unscaled_outputs`` (else ``outputs`` un-standardised)
        over the cells of ``active_entries``; ``plan``: None (the dataset's own treatments) or a plan of
        ``treatment_effect``.  One launch of ``ops.ensemble_score``: the [N, R, T] replicate rollouts never exist in
        memory.  The ensemble carries the model's uncertainty only: on noisy outcomes under-coverage is the honest
        answer."""
        coef = self._effect_coef("score_bands")
        d = dataset.data
        N = d["current_treatments"].shape[0]
        group, n_groups = self._groups(groups, N)
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arm = self._plan_arms(dataset, plan, "plan")
        if "unscaled_outputs" in d:
            y_obs = torch.as_tensor(np.ascontiguousarray(d["unscaled_outputs"][..., 0], dtype=np.float64),
                                    device=self.device)
        else:
            y_obs = torch.as_tensor(np.ascontiguousarray(d["outputs"][..., 0], dtype=np.float64),
                                    device=self.device) * std + mean
        active = torch.as_tensor(np.ascontiguousarray(d["active_entries"][..., 0] != 0).astype(np.int8),
                                 device=self.device)
        sums = ops.ensemble_score(prev[:, 0].contiguous(), stat, arm, y_obs, active, coef, self.library, self.dt,
                                  levels, n_bins=n_bins, group=group, n_groups=n_groups, method=self.integrator,
                                  drop_below=0.0, T=arm.size(1))
        return effect.from_score(sums, levels, n_bins, scale=std)

    # ------------------------------------------------------------------ regimen choice
    def _objective_weights(self, dataset, objective):
        """The step weights of ``choose_plan``: f64 [T] or [N, T] on the host."""
        ae = np.asarray(dataset.data["active_entries"][..., 0], dtype=np.float64)
        N, T = ae.shape
        if isinstance(objective, str):
            if objective == "mean":
                tot = ae.sum(axis=1, keepdims=True)
                return np.divide(ae, tot, out=np.zeros_like(ae), where=tot > 0)
            if objective == "terminal":
                w = np.zeros_like(ae)
                has = (ae > 0).any(axis=1)
                last = T - 1 - np.argmax(ae[:, ::-1] > 0, axis=1)
                w[np.nonzero(has)[0], last[has]] = 1.0
                return w
            raise ValueError("objective must be 'mean', 'terminal', an array [T] or an array [N, T]")
        w = objective.detach().cpu().numpy() if isinstance(objective, torch.Tensor) else np.asarray(objective)
        if w.shape not in ((T,), (N, T)):
            raise ValueError(f"objective must be 'mean', 'terminal', an array [{T}] or an array [{N}, {T}]")
        return w.astype(np.float64)

    def choose_plan(self, dataset, plans, objective="mean", costs=None, maximize=False,
                    quantiles=(0.025, 0.5, 0.975)):
        """Which of the candidate ``plans`` is best for every row of ``dataset``, and how sure the bootstrap ensemble
        is of it.  ``plans``: a list of 1..16 plans, each as ``treatment_effect`` takes them (None, an int, an int
        array [N, T] or a one-hot array [N, T, A]).  The objective of a plan is cost + sum_k w[p, k] y[p, k] over its
        predicted trajectory (standardised like ``get_predictions``): ``objective`` "mean" (the mean over the row's
        active entries), "terminal" (the row's last active step), or weights [T] / [N, T]; ``costs``: one number per
        plan in the same units; the smallest objective wins (the largest with ``maximize``).  The best plan is taken
        inside each bootstrap replicate, so ``win`` is the share of replicates in which a plan is the best -- not
        recoverable from per-plan or pairwise bands.  Returns an ``effect.RegimenChoiceResult``: ``choice`` (the
        point model's plan), ``win`` [N, K] and per plan the series "value" and "regret" (against the replicate's own
        best plan; divided by the output's standard deviation only).  One launch of ``ops.regimen_choice``."""
        coef = self._effect_coef("choose_plan")
        if not isinstance(plans, (list, tuple)) or not 1 <= len(plans) <= _lib.REGIMEN_MAX_PLANS:
            raise ValueError(f"choose_plan: plans must be a list of 1 to {_lib.REGIMEN_MAX_PLANS} plans")
        K = len(plans)
        if costs is not None and np.asarray(costs, dtype=np.float64).shape != (K,):
            raise ValueError(f"choose_plan: costs must hold one number per plan ({K})")
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arms = torch.stack([self._plan_arms(dataset, pl, f"plans[{j}]") for j, pl in enumerate(plans)]).contiguous()
        w = torch.as_tensor(np.ascontiguousarray(self._objective_weights(dataset, objective)), device=self.device)
        cost = None
        if costs is not None:
            cost = torch.as_tensor(np.asarray(costs, dtype=np.float64) * std, device=self.device)
        choice, win, out = ops.regimen_choice(prev[:, 0].contiguous(), stat, arms, coef, self.library, self.dt,
                                              quantiles, w, cost=cost, maximize=maximize, method=self.integrator,
                                              drop_below=0.0, T=arms.size(2))
        shift = mean * w.sum(dim=-1)                # a number (shared weights) or [N]
        return effect.from_regimen(choice, win, out, quantiles, shift=shift if w.dim() == 2 else float(shift),
                                   scale=std)

    # ------------------------------------------------------------------ closed-loop rules
    def _rule_table(self, what, dataset, rules, costs, arm_costs, max_rules):
        """A list of ``effect.ThresholdRule`` -> (the host table [(arm_on, arm_off, every, start_on)], the thresholds
        [N, 2 K] in the units of ``get_predictions``), with the checks of ``costs`` and ``arm_costs``."""
        if (not isinstance(rules, (list, tuple)) or not 1 <= len(rules) <= max_rules
                or not all(isinstance(r, effect.ThresholdRule) for r in rules)):
            raise ValueError(f"{what}: rules must be a list of 1 to {max_rules} "
                             "effect.ThresholdRule")
        K = len(rules)
        if costs is not None and np.asarray(costs, dtype=np.float64).shape != (K,):
            raise ValueError(f"{what}: costs must hold one number per rule ({K})")
        A = self.dim_treatments
        if arm_costs is not None and np.asarray(arm_costs, dtype=np.float64).shape != (A,):
            raise ValueError(f"{what}: arm_costs must hold one number per arm ({A})")
        N = dataset.data["current_treatments"].shape[0]
        table, th = [], np.empty((N, 2 * K))
        for j, r in enumerate(rules):
            if not (0 <= int(r.arm_on) < A and 0 <= int(r.arm_off) < A) or int(r.every) < 1:
                raise ValueError(f"{what}: rules[{j}]: arms must lie in [0, {A}) and every must be >= 1")
            table.append((int(r.arm_on), int(r.arm_off), int(r.every), 1 if r.start_on else 0))
            for c, v in ((2 * j, r.on), (2 * j + 1, r.on if r.off is None else r.off)):
                v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)
                if v.shape not in ((), (N,)):
                    raise ValueError(f"{what}: rules[{j}]: a threshold is a number or an array [{N}]")
                th[:, c] = v
        return table, th

    def evaluate_rules(self, dataset, rules, objective="mean", costs=None, arm_costs=None, maximize=False,
                       quantiles=(0.025, 0.5, 0.975), schedule=False):
        """How each of the closed-loop ``rules`` does for every row of ``dataset``, and how sure the bootstrap ensemble
        is of it.  ``rules``: a list of 1..16 ``effect.ThresholdRule`` -- "treat (arm_on) while the predicted state is
        at or above a threshold", decided every ``every`` steps on the state the model itself predicts, so every
        bootstrap replicate follows its own treatment sequence.  Thresholds are in the units of ``get_predictions``
        (numbers, or one per row).  ``objective``, ``costs`` (one per rule) and ``maximize`` are ``choose_plan``'s;
        ``arm_costs``: one number per arm in the same units, charged for every step spent under that arm (the
        exposure of a rule is not known in advance, so it cannot be part of ``costs``).  Returns an
        ``effect.FeedbackResult``: ``choice`` (the point model's rule), ``win`` [N, K] and per rule the series "value"
        and "regret" (``choose_plan``'s units) and "exposure" (the number of steps spent on arm_on, with its own band);
        with ``schedule`` also the arms the point model applies, int8 [N, K, T], which ``treatment_effect`` and
        ``choose_plan`` take as plans.  One launch of ``ops.feedback_rules``."""
        coef = self._effect_coef("evaluate_rules", _lib.FEEDBACK_MAX_REPLICATES)
        table, th = self._rule_table("evaluate_rules", dataset, rules, costs, arm_costs, _lib.FEEDBACK_MAX_RULES)
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        theta = torch.as_tensor(th * std + mean, device=self.device)
        w = torch.as_tensor(np.ascontiguousarray(self._objective_weights(dataset, objective)), device=self.device)
        cost = None
        if costs is not None:
            cost = torch.as_tensor(np.asarray(costs, dtype=np.float64) * std, device=self.device)
        ac = None if arm_costs is None else np.asarray(arm_costs, dtype=np.float64) * std
        choice, win, out, sched = ops.feedback_rules(prev[:, 0].contiguous(), stat, theta, table, coef, self.library,
                                                     self.dt, quantiles, w, cost=cost, arm_cost=ac, maximize=maximize,
                                                     method=self.integrator, drop_below=0.0, T=w.size(-1),
                                                     sched=True if schedule else None)
        shift = mean * w.sum(dim=-1)                # a number (shared weights) or [N]
        return effect.from_feedback(choice, win, out, quantiles, schedule=sched,
                                    shift=shift if w.dim() == 2 else float(shift), scale=std)

    # ------------------------------------------------------------------ cohort averages
    def _groups(self, groups, N):
        """``groups`` None (one group) or int ids [N] (negative: the row is excluded) -> (int32 device tensor or None,
        n_groups)."""
        if groups is None:
            return None, 1
        g = groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
        if g.shape != (N,) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"groups: expected None or an int array [{N}] of group ids")
        n_groups = int(g.max()) + 1 if g.size else 1
        if not 1 <= n_groups <= _lib.COHORT_MAX_GROUPS:
            raise ValueError(f"groups: ids must lie in [0, {_lib.COHORT_MAX_GROUPS}) with at least one row included "
                             "(negative ids exclude a row)")
        g = np.where(g < 0, -1, g).astype(np.int32)
        return torch.as_tensor(np.ascontiguousarray(g), device=self.device), n_groups

    def average_effect(self, dataset, plan_b, plan_a=None, groups=None, quantiles=(0.025, 0.5, 0.975),
                       resample="paired", seed=None):
        """The average over the cohort (ATE) and over subgroups (CATE) of the trajectories under ``plan_a`` and
        ``plan_b`` and of their difference a - b, with bands from ``bootstrap_``: every replicate averages its own
        trajectories, so the band is the band of the mean, not the mean of the rows' bands.  Plans are
        ``treatment_effect``'s.  ``groups``: None (one group) or int ids [N] (``n_groups = max + 1`` <= 64; a
        negative id excludes the row).  ``resample``: "paired" -- replicate r weighs the rows with the Poisson counts
        its own refit drew (``bootstrap_.seed``): for the training cohort in its training order; "independent" --
        Poisson counts under ``seed`` (required, different from ``bootstrap_.seed``): sampling uncertainty of a cohort
        the bootstrap never saw; None -- every weight 1: model uncertainty only.  Returns an
        ``effect.CohortEffectResult`` with the series "a", "b" and "effect": a and b standardised like
        ``get_predictions``, the effect divided by the output's standard deviation only.  One plan alone is
        ``predict_average``."""
        if plan_b is None and plan_a is None:
            raise ValueError("average_effect compares two plans: with both None they are the dataset's own "
                             "treatments twice; predict_average gives the one series of one plan")
        return self._cohort_average("average_effect", dataset, plan_a, plan_b, True, groups, quantiles, resample, seed)

    def predict_average(self, dataset, groups=None, plan=None, quantiles=(0.025, 0.5, 0.975), resample="paired",
                        seed=None):
        """``average_effect`` for one plan (None: the dataset's own treatments): the one series "a"."""
        return self._cohort_average("predict_average", dataset, plan, None, False, groups, quantiles, resample, seed)

    def _resample(self, what, resample, seed):
        """``resample`` / ``seed`` of the cohort-level calls -> (the row weighting, the seed of the Poisson counts)."""
        bs = self.bootstrap_
        if resample == "paired":
            if bs.seed is None:
                raise ValueError(f"{what}: resample='paired' needs the seed of bootstrap() (bootstrap_.seed is None)")
            weighting, use_seed = "poisson", int(bs.seed)
        elif resample == "independent":
            if seed is None or (bs.seed is not None and int(seed) == int(bs.seed)):
                raise ValueError(f"{what}: resample='independent' needs a seed, different from bootstrap_.seed")
            weighting, use_seed = "poisson", int(seed)
        elif resample is None:
            weighting, use_seed = "none", 0
        else:
            raise ValueError(f"{what}: resample must be 'paired', 'independent' or None")
        return weighting, use_seed

    def _cohort_average(self, what, dataset, plan_a, plan_b, two, groups, quantiles, resample, seed):
        coef = self._effect_coef(what, _lib.COHORT_MAX_REPLICATES)
        weighting, use_seed = self._resample(what, resample, seed)
        N = dataset.data["current_treatments"].shape[0]
        group, n_groups = self._groups(groups, N)
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arm_a = self._plan_arms(dataset, plan_a, "plan_a" if two else "plan")
        arm_b = self._plan_arms(dataset, plan_b, "plan_b") if two else None
        out, _, wsum = ops.cohort_effect(prev[:, 0].contiguous(), stat, arm_a, arm_b, coef, self.library, self.dt,
                                         quantiles, group=group, n_groups=n_groups, weighting=weighting,
                                         seed=use_seed, method=self.integrator, drop_below=0.0, T=arm_a.size(1))
        return effect.from_cohort(out, wsum, quantiles, shift=mean, scale=std)

    # ------------------------------------------------------------------ policy value
    def _cohort_objective(self, what, dataset, objective, groups):
        """The step weights of a cohort value and what their shift needs: (w f64 [T] or [N, T] on the host, the one
        sum_k w of the cohort, the group ids with the rows that have no active entry excluded)."""
        N = dataset.data["current_treatments"].shape[0]
        w = self._objective_weights(dataset, objective)
        tot = np.broadcast_to(w.sum(axis=-1), (N,)) if w.ndim == 2 else np.full(N, w.sum())
        g = None if groups is None else (groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor)
                                         else np.asarray(groups))
        if isinstance(objective, str):
            # a row with no active entry has no objective: excluded (its weights are all zero)
            empty = ~(np.asarray(dataset.data["active_entries"][..., 0]) > 0).any(axis=1)
            if empty.any():
                if g is None:
                    g = np.zeros(N, dtype=np.int64)
                elif g.shape != (N,) or not np.issubdtype(g.dtype, np.integer):
                    raise ValueError(f"groups: expected None or an int array [{N}] of group ids")
                g = np.where(empty, -1, g)
            tot = tot[~empty]
        wtot = float(tot[0]) if tot.size else 0.0
        if tot.size and float(np.max(tot) - np.min(tot)) > 1e-12 * max(float(np.max(np.abs(tot))), 1e-300):
            raise ValueError(f"{what}: the rows of an [N, T] objective must all have the same sum (the cohort "
                             "value is standardised with one sum_k w): normalise every row's weights to one total")
        return w, wtot, g

    def policy_value(self, dataset, plans, rule=None, objective="mean", costs=None, maximize=False, groups=None,
                     quantiles=(0.025, 0.5, 0.975), resample="paired", seed=None):
        """What the cohort (and every subgroup) gains if every row gets its own best plan of ``plans`` instead of
        everyone getting the best single plan, with bands from ``bootstrap_``.  ``plans``, ``objective``, ``costs``
        and ``maximize`` are ``choose_plan``'s; ``groups``, ``resample`` and ``seed`` are ``average_effect``'s.
        ``rule``: None (the point model's choice, ``choose_plan(...).choice``) or an int array [N] of plan indices
        in [0, K): the fixed per-row rule that every replicate's model evaluates -- its value is free of the
        optimism of an argmin re-derived inside the replicate, which the series "optimism" measures.  Returns an
        ``effect.PolicyValueResult``: the series value_j, personalised, rule and best_fixed in ``choose_plan``'s
        units ((J - mean sum_k w) / std), gain_personalised, gain_rule and optimism divided by the output's standard
        deviation only, share_j unitless.  The shift needs one sum_k w for the whole cohort, so an [N, T]
        ``objective`` whose rows do not all have the same sum is refused; under "mean" / "terminal" a row with no
        active entry is excluded as a negative group id excludes it.  One launch of ``ops.policy_value``."""
        coef = self._effect_coef("policy_value", _lib.POLICY_MAX_REPLICATES)
        weighting, use_seed = self._resample("policy_value", resample, seed)
        if not isinstance(plans, (list, tuple)) or not 1 <= len(plans) <= _lib.POLICY_MAX_PLANS:
            raise ValueError(f"policy_value: plans must be a list of 1 to {_lib.POLICY_MAX_PLANS} plans")
        K = len(plans)
        if costs is not None and np.asarray(costs, dtype=np.float64).shape != (K,):
            raise ValueError(f"policy_value: costs must hold one number per plan ({K})")
        N = dataset.data["current_treatments"].shape[0]
        rule_t = None
        if rule is not None:
            rl = rule.detach().cpu().numpy() if isinstance(rule, torch.Tensor) else np.asarray(rule)
            if rl.shape != (N,) or not np.issubdtype(rl.dtype, np.integer) or (rl.size and (rl.min() < 0
                                                                                          or rl.max() >= K)):
                raise ValueError(f"policy_value: rule must be None or an int array [{N}] of plan indices in [0, {K})")
            rule_t = torch.as_tensor(np.ascontiguousarray(rl.astype(np.int32)), device=self.device)
        w, wtot, g = self._cohort_objective("policy_value", dataset, objective, groups)
        group, n_groups = self._groups(g, N)
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        arms = torch.stack([self._plan_arms(dataset, pl, f"plans[{j}]") for j, pl in enumerate(plans)]).contiguous()
        wt = torch.as_tensor(np.ascontiguousarray(w), device=self.device)
        cost = None
        if costs is not None:
            cost = torch.as_tensor(np.asarray(costs, dtype=np.float64) * std, device=self.device)
        out, fixwin, best_fixed, rule_o, _, wsum = ops.policy_value(
            prev[:, 0].contiguous(), stat, arms, coef, self.library, self.dt, quantiles, wt, cost=cost,
            maximize=maximize, rule=rule_t, group=group, n_groups=n_groups, weighting=weighting, seed=use_seed,
            method=self.integrator, drop_below=0.0, T=arms.size(2))
        return effect.from_policy(out, fixwin, best_fixed, rule_o, wsum, quantiles, shift=mean * wtot, scale=std)

    # ------------------------------------------------------------------ rule value
    def rule_value(self, dataset, rules, assignment=None, objective="mean", costs=None, arm_costs=None,
                   maximize=False, groups=None, quantiles=(0.025, 0.5, 0.975), resample="paired", seed=None):
        """What the cohort (and every subgroup) gains under each of the closed-loop ``rules``, what it gains if every
        row gets its own best rule instead of everyone following the best single rule, and how many treated steps
        per row each policy costs, with bands from ``bootstrap_``.  ``rules``, ``objective``, ``costs``,
        ``arm_costs`` and ``maximize`` are ``evaluate_rules``'; ``groups``, ``resample`` and ``seed`` are
        ``average_effect``'s.  ``assignment``: None (the point model's choice, ``evaluate_rules(...).choice``) or an
        int array [N] of rule indices in [0, K): the fixed per-row assignment that every replicate's model evaluates.
        Returns an ``effect.RuleValueResult``: the series value_j, personalised, assigned and best_fixed in
        ``evaluate_rules``' units ((J - mean sum_k w) / std), gain_personalised, gain_assigned and optimism divided by
        the output's standard deviation only, share_j and the exposures (treated steps per row) not rescaled.  An
        [N, T] ``objective`` whose rows do not all have the same sum is refused; under "mean" / "terminal" a row with
        no active entry is excluded, as in ``policy_value``.  One launch of ``ops.rule_value``."""
        coef = self._effect_coef("rule_value", _lib.RULEVALUE_MAX_REPLICATES)
        weighting, use_seed = self._resample("rule_value", resample, seed)
        table, th = self._rule_table("rule_value", dataset, rules, costs, arm_costs, _lib.RULEVALUE_MAX_RULES)
        K = len(table)
        N = dataset.data["current_treatments"].shape[0]
        assign_t = None
        if assignment is not None:
            al = assignment.detach().cpu().numpy() if isinstance(assignment, torch.Tensor) else np.asarray(assignment)
            if al.shape != (N,) or not np.issubdtype(al.dtype, np.integer) or (al.size and (al.min() < 0
                                                                                          or al.max() >= K)):
                raise ValueError(f"rule_value: assignment must be None or an int array [{N}] of rule indices in "
                                 f"[0, {K})")
            assign_t = torch.as_tensor(np.ascontiguousarray(al.astype(np.int32)), device=self.device)
        w, wtot, g = self._cohort_objective("rule_value", dataset, objective, groups)
        group, n_groups = self._groups(g, N)
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        theta = torch.as_tensor(th * std + mean, device=self.device)
        wt = torch.as_tensor(np.ascontiguousarray(w), device=self.device)
        cost = None
        if costs is not None:
            cost = torch.as_tensor(np.asarray(costs, dtype=np.float64) * std, device=self.device)
        ac = None if arm_costs is None else np.asarray(arm_costs, dtype=np.float64) * std
        out, fixwin, best_fixed, assign_o, _, wsum = ops.rule_value(
            prev[:, 0].contiguous(), stat, theta, table, coef, self.library, self.dt, quantiles, wt, cost=cost,
            arm_cost=ac, maximize=maximize, assign=assign_t, group=group, n_groups=n_groups, weighting=weighting,
            seed=use_seed, method=self.integrator, drop_below=0.0, T=wt.size(-1))
        return effect.from_rule_value(out, fixwin, best_fixed, assign_o, wsum, quantiles, shift=mean * wtot,
                                      scale=std)

    # ------------------------------------------------------------------ rollout (A8)
    def _predict_device(self, dataset, tau=1):
        """Standardised open-loop predictions [N, T-1] on the device (sindy.py:371-431); with
        ``insite`` the per-patient refined predictions (get_predictions passes the reference's default
        projection_horizon=1, the autoregressive path the dataset's tau; sindy.py:362-369, 736-738)."""
        if self.insite:
            return self._refined_device(dataset, tau)
        if self._coef_dev is None:
            raise RuntimeError("fit() first")
        d = dataset.data
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        T = d["prev_outputs"].shape[1]
        if self.joint_model:   # per-step treatment combination = the folded model's arm
            arm = torch.as_tensor(self._treatment_code(d["current_treatments"]), device=self.device)
        else:
            arm = torch.as_tensor(np.argmax(d["current_treatments"], axis=-1).astype(np.int8), device=self.device)
        y = ops.rollout(prev[:, 0].contiguous(), stat, arm.contiguous(), self._coef_dev, self._roll_library, self.dt,
                        method=self.integrator, drop_below=0.0, T=T)
        return (y - mean) / std

    def _refined_device(self, dataset, tau):
        """INSITE predictions (sindy.py:433-715): every row with sequence_length > tau refines the active
        global coefficients by BFGS on its own observed prefix (insite_refine_f64, one lane per row),
        then rolls its refined model out with the reference's Euler-5 odeint.  Standardised [N, T]."""
        if self.joint_coefs is None:
            raise RuntimeError("fit() first")
        if self.lam is None:
            raise ValueError("model.lam must be set for insite: true (reference config: 10.0 for EQ_4)")
        d = dataset.data
        prev, stat, std, mean = self._unscaled_inputs(dataset)
        if self.smooth_input_data:      # applied here in the reference (sindy.py:557-560), unlike the DE format
            prev = savgol_5_3_rows(prev)
        if self.segment_mode and "EQ_5" in self.dataset_name.upper() and stat.shape[1] >= 2:
            # the reference's EQ_5 refinement binds u1 to static_features[0] (sindy.py:536), unlike its
            # global-model rollout (sindy.py:302): kept, so refined EQ_5 predictions match the reference
            stat = stat[:, :1].expand(-1, stat.shape[1]).contiguous()
        if self.joint_model:   # the per-step treatment bit code selects the folded combination (sindy.py:469-551)
            arm = torch.as_tensor(self._treatment_code(d["current_treatments"]), device=self.device)
        else:
            arm = torch.as_tensor(np.argmax(d["current_treatments"], axis=-1).astype(np.int8), device=self.device)
        sl = torch.as_tensor(np.asarray(d["sequence_lengths"]).astype(np.int32), device=self.device)
        preds, coef, status, iters = ops.insite_refine(prev.contiguous(), arm.contiguous(), stat, sl, self.joint_coefs,
                                                       self.library, self.dt, float(self.lam), int(tau), substeps=5,
                                                       revert_on_zoom_fail=self.insite_revert_on_zoom_fail)
        self.insite_status, self.insite_iters, self.insite_coefs = status, iters, coef
        scaled = ((preds - mean) / std).contiguous()
        # the reference refuses refined predictions with NaN or Inf (sindy.py:710): a refined model that blows up
        # inside the row's horizon ends the run there, not in a metric later
        if not bool(torch.isfinite(scaled).all()):
            raise AssertionError("Scaled_preds contains NaN or Inf")
        return scaled

    def get_predictions(self, dataset) -> np.ndarray:
        logger.info("Predictions for %s.", getattr(dataset, "subset_name", "?"))
        p = self._predict_device(dataset).cpu().numpy()[..., None]
        assert not np.any(np.isnan(p)), "Predictions contains NaN"
        return p

    def _slice_device(self, pred, dataset, offset=1):
        """tau-step window per row from max(offset, seq_len - tau) (sindy.py:729-733), with
        jax.lax.dynamic_slice's clamp to [0, T - tau]."""
        tau = self.projection_horizon
        T = pred.shape[1]
        sl = torch.as_tensor(np.asarray(dataset.data["sequence_lengths"]).astype(np.int64), device=pred.device)
        lo = torch.clamp(torch.clamp(sl - tau, min=offset), 0, T - tau)
        idx = lo[:, None] + torch.arange(tau, device=pred.device)[None, :]
        return torch.gather(pred, 1, idx)

    def get_autoregressive_predictions(self, dataset) -> np.ndarray:
        logger.info("Autoregressive Prediction for %s.", getattr(dataset, "subset_name", "?"))
        pred = self._predict_device(dataset, tau=self.projection_horizon)
        return self._slice_device(pred, dataset).cpu().numpy()[..., None]

    # ------------------------------------------------------------------ metrics (A10)
    def _sse(self, pred_scaled, target, active, std, mean):
        """Masked squared-error sums on the device; the prediction is un-scaled in the kernel
        (pred * std + mean, as time_varying_model.py:249) when ``unscale_rmse``."""
        tgt = torch.as_tensor(np.ascontiguousarray(target), device=pred_scaled.device)
        act = torch.as_tensor(np.ascontiguousarray(active), device=pred_scaled.device)
        if self.unscale_rmse:
            return ops.masked_sse(pred_scaled.contiguous(), tgt, act, scale=std, shift=mean)
        return ops.masked_sse(pred_scaled.contiguous(), tgt, act)

    def get_normalised_masked_rmse(self, dataset, one_step_counterfactual=False):
        logger.info("RMSE calculation for %s.", getattr(dataset, "subset_name", "?"))
        sp = dataset.scaling_params
        std, mean = float(sp["output_stds"]), float(sp["output_means"])
        pred = self._predict_device(dataset)
        if torch.isnan(pred).any():
            raise AssertionError("Predictions contains NaN")
        key = "unscaled_outputs" if self.unscale_rmse else "outputs"
        per, cnt, last = self._sse(pred, dataset.data[key][..., 0], dataset.data["active_entries"][..., 0], std, mean)
        per, cnt, last = per.cpu().numpy(), cnt.cpu().numpy(), last.cpu().numpy()
        norm = dataset.norm_const
        scale = 100.0 if self.percentage_rmse else 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            orig = np.sqrt((per / cnt).mean()) / norm * scale
            allv = np.sqrt(per.sum() / cnt.sum()) / norm * scale
            if not one_step_counterfactual:
                return orig, allv
            lastv = np.sqrt(last[0] / last[1]) / norm * scale
        return orig, allv, lastv

    def get_normalised_n_step_rmses(self, dataset, datasets_mc=None):
        logger.info("RMSE calculation for %s.", getattr(dataset, "subset_name", "?"))
        seq = dataset.data_processed_seq
        assert seq is not None, "dataset has no data_processed_seq (process_data_multi first)"
        sp = dataset.scaling_params
        std, mean = float(sp["output_stds"]), float(sp["output_means"])
        pred = self._slice_device(self._predict_device(dataset if datasets_mc is None else datasets_mc,
                                                       tau=self.projection_horizon), dataset)
        key = "unscaled_outputs" if self.unscale_rmse else "outputs"
        not_nan = ~np.isnan(seq["outputs"][..., 0]).any(axis=1)          # time_varying_model.py:302-303
        idx = torch.as_tensor(np.nonzero(not_nan)[0], device=pred.device)
        per, cnt, _ = self._sse(pred.index_select(0, idx), seq[key][not_nan][..., 0],
                                seq["active_entries"][not_nan][..., 0], std, mean)
        per, cnt = per.cpu().numpy(), cnt.cpu().numpy()
        r = np.sqrt(per / cnt) / dataset.norm_const
        return r * (100.0 if self.percentage_rmse else 1.0)
