"""The entries of Context that the statistics part of the library implements: compare, the two-sample family, nested
R-hat, Pareto k-hat, PSIS / LOO, HDI, weighted summaries, SBC ranks, autocorrelation and covariance.  A base of Context
(see _context.py).
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from ._abi import ENERGY_KEYS, MCR_ACF_MAX_LAG, MCR_ACF_UNBIASED, _as_dp, _as_ip, tensor4_args, tensor_args, thin_args
from ._device import DeviceBuffer, DeviceSims, DeviceTensor
from ._hostdefs import (_acf_arrays, _acf_result, _hdi_arrays, _nan_arrays, _nested_arrays, _pareto_arrays, _psis_arrays,
                        _sample_pair, _sbc_arrays, _truth_array, _weighted_arrays, loo_totals, pareto_companions,
                        pareto_tail_length, superchain_labels, weight_arguments)


def _void_p(v) -> C.c_void_p:
    """A device address given as an int or as a c_void_p (DeviceBuffer.ptr)."""
    return v if isinstance(v, C.c_void_p) else C.c_void_p(int(v))


class _StatCalls:
    """The statistics entries: what mcr_api.hip and mcr_stats.hip implement."""

    def compare(self, ref, actual, tol: float):
        r = np.ascontiguousarray(ref, dtype=np.float64)
        a = np.ascontiguousarray(actual, dtype=np.float64)
        if r.shape != a.shape:
            raise ValueError("ref and actual must have the same shape")
        rel = np.empty(max(r.size, 1))
        ok = np.zeros(max(r.size, 1), dtype=np.uint8)
        self._check(self.lib.mcr_compare(self.handle, _as_dp(r), _as_dp(a), r.size, float(tol), _as_dp(rel),
                                         ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return rel[:r.size], ok[:r.size].astype(bool)

    # -- extensions (not in the reference) -------------------------------------------------------------
    def two_sample(self, ref, actual) -> tuple[np.ndarray, np.ndarray]:
        """(KS statistic, Wasserstein-1) per parameter; ref [P][Mr], actual [P][Ma] (2-D, finite)."""
        r, a = _sample_pair(ref, actual)
        P = r.shape[0]
        ks, w1 = _nan_arrays(("ks", "w1"), P).values()
        self._check(self.lib.mcr_two_sample(self.handle, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], P,
                                            _as_dp(ks), _as_dp(w1)))
        return ks[:P], w1[:P]

    @staticmethod
    def _sliced_args(directions, center, P: int):
        w = np.ascontiguousarray(directions, dtype=np.float64)
        if w.ndim != 2 or (w.shape[0] and w.shape[1] != P):
            raise ValueError("directions must be 2-D [K][P] with one weight per parameter")
        c = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
        if c is not None and c.shape != (P,):
            raise ValueError("center must have one entry per parameter")
        if not (np.isfinite(w).all() and (c is None or np.isfinite(c).all())):
            raise ValueError("directions and center must be finite")
        return w, c

    def sliced_two_sample(self, ref, actual, directions, center=None, projections: bool = False):
        """(KS statistic, Wasserstein-1) per direction of the two samples projected onto `directions` [K][P]:
        z[k] = sum_p directions[k][p] * (x[p] - center[p]), p in order, one fma each (mcr_sliced_two_sample).  ref [P][Mr],
        actual [P][Ma] (2-D, finite); center [P] or None for zeros.  projections=True appends the projected rows
        zr [K][Mr], za [K][Ma]."""
        r, a = _sample_pair(ref, actual)
        w, c = self._sliced_args(directions, center, r.shape[0])
        return self._sliced(self.lib.mcr_sliced_two_sample, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], w, c,
                            projections)

    def sliced_two_sample_dev(self, ref_ptr, Mr: int, act_ptr, Ma: int, P: int, directions, center=None,
                              projections: bool = False):
        """sliced_two_sample on draws already in this context's device memory: ref_ptr -> [P][Mr] f64, act_ptr -> [P][Ma]
        f64 (device addresses or DeviceBuffer.ptr).  Non-finite draws raise McrError (MCR_ENONFINITE)."""
        w, c = self._sliced_args(directions, center, P)
        return self._sliced(self.lib.mcr_sliced_two_sample_dev, _void_p(ref_ptr), int(Mr), _void_p(act_ptr), int(Ma), int(P), w, c,
                            projections)

    def _sliced(self, entry, ref, Mr, act, Ma, P, w, c, projections):
        K = w.shape[0]
        ks, w1 = _nan_arrays(("ks", "w1"), K).values()
        zr = np.empty((K, Mr)) if projections else None
        za = np.empty((K, Ma)) if projections else None
        self._check(entry(self.handle, ref, Mr, act, Ma, P, _as_dp(w), _as_dp(c), K, _as_dp(ks), _as_dp(w1),
                          _as_dp(zr), _as_dp(za)))
        return (ks[:K], w1[:K], zr, za) if projections else (ks[:K], w1[:K])

    def sliced_dirs_per_chunk(self, Mr: int, Ma: int, P: int, K: int) -> int:
        """Directions per workspace chunk of a sliced_two_sample call of this shape (mcr_sliced_plan)."""
        return self._answer("mcr_sliced_plan", Mr, Ma, P, K)

    @staticmethod
    def _energy_scale(scale, P: int):
        s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        if s is not None and s.shape != (P,):
            raise ValueError("scale must have one entry per parameter")
        if s is not None and not (np.isfinite(s).all() and (s >= 0).all()):
            raise ValueError("scale must be finite and >= 0")
        return s

    def energy_distance(self, ref, actual, scale=None) -> dict:
        """Energy distance of Szekely and Rizzo between the joint draws ref [P][Mr] and actual [P][Ma] (2-D, finite), every
        parameter multiplied by scale[p] first (None: ones) -- mcr_energy_distance.  Keys: a, b, c (the mean distances
        between the samples, within ref, within actual), e = 2a - b - c, h = e / 2a in [0, 1], t = Mr Ma / (Mr + Ma) e."""
        r, a = _sample_pair(ref, actual)
        s = self._energy_scale(scale, r.shape[0])
        return self._energy(self.lib.mcr_energy_distance, _as_dp(r), r.shape[1], _as_dp(a), a.shape[1], r.shape[0], s)

    def energy_distance_dev(self, ref_ptr, Mr: int, act_ptr, Ma: int, P: int, scale=None) -> dict:
        """energy_distance on draws already in this context's device memory: ref_ptr -> [P][Mr] f64, act_ptr -> [P][Ma]
        f64 (device addresses or DeviceBuffer.ptr).  Non-finite draws raise McrError (MCR_ENONFINITE)."""
        s = self._energy_scale(scale, int(P))
        return self._energy(self.lib.mcr_energy_distance_dev, _void_p(ref_ptr), int(Mr), _void_p(act_ptr), int(Ma), int(P), s)

    def _energy(self, entry, ref, Mr, act, Ma, P, s) -> dict:
        out = np.full(6, np.nan)
        self._check(entry(self.handle, ref, Mr, act, Ma, P, _as_dp(s), _as_dp(out)))
        return dict(zip(ENERGY_KEYS, (float(v) for v in out)))

    def energy_workspace(self, Mr: int, Ma: int, P: int) -> int:
        """Bytes of workspace an energy_distance call of this shape carves (mcr_energy_workspace)."""
        v = C.c_size_t(0)
        self._check(self.lib.mcr_energy_workspace(self.handle, int(Mr), int(Ma), int(P), C.byref(v)))
        return int(v.value)

    def nested_rhat(self, draws, superchain_ids, layout: str = "pcn") -> dict:
        """Nested R-hat per parameter (mcr_nested_rhat: Margossian et al., posterior::rhat_nested) of a host array or a
        DeviceTensor with any number of chains up to MCR_NESTED_MAX_CHAINS.  superchain_ids: one integer label per chain
        (any labels, every one equally often), or an int K for K contiguous blocks of C / K chains.  Arrays per
        parameter: nrhat = max(nrhat_bulk, nrhat_tail), nrhat_raw (the paper's, on the draws), between_* / within_* (B and
        W of each kind).  Chains are not split."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "nested_rhat", False)
        ids = superchain_labels(superchain_ids, targs[1])
        arrs, out = _nested_arrays(targs[3])
        self._check(fn(self.handle, ptr, *targs, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(out)))
        return {n: a[:targs[3]] for n, a in arrs.items()}

    def nested_params_per_chunk(self, t: "DeviceTensor", K: int) -> int:
        """Parameters per workspace chunk of a nested_rhat call on this tensor with K superchains (mcr_nested_plan)."""
        return self._params_per_chunk("mcr_nested_plan", t.targs, int(K))

    _EQUAL_CHAINS = {"nested_rhat": "nested R-hat", "autocorr": "autocorrelation"}

    def _tensor_call(self, draws, layout: str, name: str, pooled: bool):
        """(targs, pointer, entry, on_device) of a call mcr_<name> on a host array or, on_device, mcr_<name>_dev on a
        DeviceTensor.  A ragged tensor is, pooled, one chain of its pooled draws; otherwise it is refused."""
        if isinstance(draws, DeviceSims):
            raise ValueError(f"{name} takes one (C, N, P) tensor; a DeviceSims holds S of them (Context.sbc_ranks)")
        if not isinstance(draws, DeviceTensor):
            return tensor_args(draws, layout), draws.ctypes.data_as(C.c_void_p), getattr(self.lib, "mcr_" + name), False
        targs = draws.targs
        if draws.chain_off is not None:
            if not pooled:
                raise ValueError(f"{self._EQUAL_CHAINS[name]} needs chains of equal length; a ragged tensor is not supported")
            M = int(draws.chain_off[-1])
            targs = (targs[0], 1, M, targs[3], M, 1, targs[6])
        return targs, draws.buf.ptr, getattr(self.lib, f"mcr_{name}_dev"), True

    def _params_per_chunk(self, plan_symbol: str, t, *extra, call: str = "", pooled: bool = False) -> int:
        """What an mcr_*_plan entry answers for a tensor and the call's own arguments: `t` is a DeviceTensor as mcr_<call>
        takes it (_tensor_call), or without `call` the tensor arguments themselves."""
        targs = self._tensor_call(t, "pcn", call, pooled)[0] if call else t
        return self._answer(plan_symbol, *targs, *extra)

    def pareto_khat(self, draws, layout: str = "pcn", r_eff=None, ndraws_tail=None) -> dict:
        """Pareto k-hat of every parameter's tails (mcr_pareto_khat: posterior::pareto_khat(tail = "both")) of a host
        array or a DeviceTensor; the chains are pooled, so a ragged tensor is accepted.  ndraws_tail: a tail length or P of
        them (>= 1); or r_eff: a relative efficiency or P of them, turned into tail lengths by mcr_pareto_tail_length;
        neither: the default of r_eff = 1.  Arrays per parameter: khat = max(khat_left, khat_right), khat_left, khat_right,
        ndraws_tail (the effective length), min_ss; and the float khat_threshold (pareto_companions)."""
        if r_eff is not None and ndraws_tail is not None:
            raise ValueError("give r_eff or ndraws_tail, not both")
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "pareto_khat", True)
        M, P = targs[1] * targs[2], targs[3]
        tails = None
        if r_eff is not None:
            r = np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (P,))
            tails = np.array([max(pareto_tail_length(M, v), 1) for v in r], dtype=np.int64)
        elif ndraws_tail is not None:
            tails = np.ascontiguousarray(np.broadcast_to(np.asarray(ndraws_tail), (P,)), dtype=np.int64)
        arrs, out = _pareto_arrays(P)
        self._check(fn(self.handle, ptr, *targs, None if tails is None else _as_ip(tails), C.byref(out)))
        res = {n: a[:P] for n, a in arrs.items()}
        res["min_ss"], res["khat_threshold"] = pareto_companions(res["khat"], M)
        return res

    def pareto_params_per_chunk(self, t: "DeviceTensor") -> int:
        """Parameters per workspace chunk of a pareto_khat call on this tensor (mcr_pareto_plan)."""
        return self._params_per_chunk("mcr_pareto_plan", t, call="pareto_khat", pooled=True)

    def _psis_call(self, draws, layout: str, negate: bool, r_eff, ndraws_tail, weights: bool) -> dict:
        """Every output of mcr_psis (a host array) or mcr_psis_dev (a DeviceTensor: the weights are written to device
        memory and fetched here); psis and loo each return their part."""
        targs, ptr, fn, dev = self._tensor_call(draws, layout, "psis", True)
        M, P = targs[1] * targs[2], targs[3]
        r = None if r_eff is None else np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (P,)))
        tails = None if ndraws_tail is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ndraws_tail), (P,)), dtype=np.int64)
        lw = np.full(max(P * M, 1), np.nan) if weights and not dev else None
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(P * M * 8, 8))) if weights and dev else None
            wptr = buf.ptr if buf is not None else lw.ctypes.data_as(C.c_void_p) if lw is not None else None
            arrs, out = _psis_arrays(P, wptr)
            self._check(fn(self.handle, ptr, *targs, int(bool(negate)), _as_dp(r), _as_ip(tails), C.byref(out)))
            if buf is not None:
                lw = buf.download(np.float64, max(P * M, 1))
        res = {n: a[:P] for n, a in arrs.items()}
        if weights:
            res["log_weights"] = lw[:P * M].reshape(P, M)
        res["min_ss"], res["khat_threshold"] = pareto_companions(res["khat"], M)
        res["n_draws"] = int(M)
        return res

    def psis(self, log_ratios, layout: str = "pcn", r_eff=None, ndraws_tail=None, weights: bool = True) -> dict:
        """Pareto-smoothed importance sampling of every column of log importance ratios (mcr_psis: ArviZ's psislw, loo::psis)
        of a host array or a DeviceTensor; the chains are pooled, so a ragged tensor is accepted.  r_eff: a relative
        efficiency or P of them (default 1); ndraws_tail: a tail length or P of them (>= 1) instead of the default.
        "log_weights" [P][M] in time order (normalised: every row's exp sums to 1; left out with weights=False, when
        k_psis_weights does not run), and per column "khat", "ndraws_tail" (the tail values actually smoothed over),
        "min_ss"; the float "khat_threshold" (pareto_companions)."""
        if r_eff is not None and ndraws_tail is not None:
            raise ValueError("give r_eff or ndraws_tail, not both")
        res = self._psis_call(log_ratios, layout, False, r_eff, ndraws_tail, weights)
        return {k: v for k, v in res.items() if k not in ("lppd", "elpd", "p_loo", "n_draws")}

    def loo(self, log_lik, layout: str = "pcn", r_eff=None, pointwise: bool = True) -> dict:
        """PSIS-LOO of a (chains x draws x observations) tensor of pointwise log-likelihoods, the observations on the
        parameter axis (mcr_psis with negate: ArviZ's loo, loo::loo).  r_eff: as in psis.  The floats "elpd_loo", "se",
        "p_loo", "lppd", the ints "n_obs" and "n_draws", "khat_counts" (loo_totals), "khat_threshold"; with pointwise also
        the arrays "elpd_i", "p_loo_i", "lppd_i", "khat" and "ndraws_tail" per observation."""
        res = self._psis_call(log_lik, layout, True, r_eff, None, False)
        out = loo_totals(res["elpd"], res["p_loo"], res["lppd"], res["khat"])
        out["n_draws"], out["khat_threshold"] = res["n_draws"], res["khat_threshold"]
        if pointwise:
            out.update({"elpd_i": res["elpd"], "p_loo_i": res["p_loo"], "lppd_i": res["lppd"], "khat": res["khat"],
                        "ndraws_tail": res["ndraws_tail"]})
        return out

    def psis_params_per_chunk(self, t: "DeviceTensor", host_weights: bool = False) -> int:
        """Columns per workspace chunk of a psis / loo call on this tensor (mcr_psis_plan); host_weights: of the host
        entry with weights, whose chunk holds them too."""
        return self._params_per_chunk("mcr_psis_plan", t, int(host_weights), call="psis", pooled=True)

    def hdi(self, draws, layout: str = "pcn", prob=0.94) -> dict:
        """Highest-density interval(s) of every parameter (mcr_hdi: ArviZ's unimodal hdi, the shortest interval holding
        floor(prob * M) + 1 of the M pooled draws) of a host array or a DeviceTensor; the chains are pooled, so a ragged
        tensor is accepted.  prob: a float, or a sequence of up to MCR_HDI_MAX_PROBS.  "lo", "hi" (float64) and "index"
        (int64, the rank of lo in the ascending order; -1 with NaN endpoints when there is no window) are [P] arrays for
        a float and [P][nprob] for a sequence; "prob" is what was asked for."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "hdi", True)
        P = targs[3]
        pr = np.ascontiguousarray(np.atleast_1d(prob), dtype=np.float64)
        if pr.ndim != 1:
            raise ValueError("prob must be a float or a flat sequence of floats")
        n = int(pr.size)
        arrs, out = _hdi_arrays(P, n)
        self._check(fn(self.handle, ptr, *targs, _as_dp(pr), n, C.byref(out)))
        res = {k: a[:P, :n] for k, a in arrs.items()}
        if np.ndim(prob) == 0:
            return {**{k: v[:, 0] for k, v in res.items()}, "prob": float(prob)}
        return {**res, "prob": pr}

    def hdi_params_per_chunk(self, t: "DeviceTensor", nprob: int = 1) -> int:
        """Parameters per workspace chunk of an hdi call with nprob probabilities on this tensor (mcr_hdi_plan)."""
        return self._params_per_chunk("mcr_hdi_plan", t, int(nprob), call="hdi", pooled=True)

    def weighted_summary(self, draws, layout: str = "pcn", *, log_weights=None, weights=None, quantiles=(0.05, 0.5, 0.95),
                         return_weights: bool = False) -> dict:
        """Importance-weighted mean, sd, standard error of the mean and quantiles of every parameter (mcr_weighted_summary:
        posterior's weight_draws + summarise_draws, numpy.quantile(weights=, method="inverted_cdf")) of a host array or a
        DeviceTensor under ONE weight per pooled draw, m = c * N + n; the chains are pooled, so a ragged tensor is
        accepted.  Exactly one of log_weights (finite or -inf; Context.psis's rows are such) and weights (finite, >= 0).
        "mean", "sd", "mean_se" [P], "quantiles" [P][nq] (inverted CDF: draws, never interpolated), the floats "ess"
        (Kish's) and "weight_sum", "n_draws"; with return_weights "weights" [M], the linear weights the call formed."""
        targs, ptr, fn, dev = self._tensor_call(draws, layout, "weighted_summary", True)
        M, P = targs[1] * targs[2], targs[3]
        v, flags, q = weight_arguments(M, log_weights, weights, quantiles)
        nq = int(q.size)
        w = np.full(max(M, 1), np.nan) if return_weights else None
        vbuf = wbuf = None
        with contextlib.ExitStack() as stack:
            if dev:
                vbuf = stack.enter_context(DeviceBuffer(self, max(M * 8, 8)))
                if M:
                    vbuf.upload(v)
                wbuf = stack.enter_context(DeviceBuffer(self, max(M * 8, 8))) if return_weights else None
            vptr = vbuf.ptr if dev else v.ctypes.data_as(C.c_void_p)
            wptr = None if w is None else wbuf.ptr if dev else w.ctypes.data_as(C.c_void_p)
            arrs, out = _weighted_arrays(P, nq, wptr)
            self._check(fn(self.handle, ptr, *targs, vptr, flags, _as_dp(q), nq, C.byref(out)))
            if wbuf is not None:
                w = wbuf.download(np.float64, max(M, 1))
        res = {n: arrs[n][:P] for n in ("mean", "sd", "mean_se")}
        res.update({"quantiles": arrs["quantiles"][:P, :nq], "ess": float(arrs["ess"][0]),
                    "weight_sum": float(arrs["weight_sum"][0]), "n_draws": int(M)})
        if return_weights:
            res["weights"] = w[:M]
        return res

    def weighted_params_per_chunk(self, t: "DeviceTensor", nq: int = 3) -> int:
        """Parameters per workspace chunk of a weighted_summary call with nq quantiles on this tensor (mcr_weighted_plan)."""
        return self._params_per_chunk("mcr_weighted_plan", t, int(nq), call="weighted_summary", pooled=True)

    def upload_sims(self, draws: np.ndarray, layout: str = "spcn") -> DeviceSims:
        """The draws of S simulations in HBM, for sbc_ranks: a 4-D C-contiguous array whose axes are `layout`."""
        targs = tensor4_args(draws, layout)
        if not draws.flags.c_contiguous:
            raise ValueError("upload_sims() needs a C-contiguous array (permute the layout string instead)")
        with contextlib.ExitStack() as stack:
            buf = stack.enter_context(DeviceBuffer(self, max(draws.nbytes, 8))).upload(draws)
            stack.pop_all()
        return DeviceSims(self, buf, targs)

    def _sbc_call(self, draws, layout: str, thin: int):
        """(thinned targs, pointer, entry) of a rank call on a 4-D host array or on the DeviceSims of S simulations."""
        if isinstance(draws, DeviceTensor):
            raise ValueError("sbc_ranks needs the DeviceSims of S simulations (Context.upload_sims), not one DeviceTensor")
        if isinstance(draws, DeviceSims):
            return thin_args(draws.targs, thin), draws.buf.ptr, self.lib.mcr_sbc_ranks_dev
        return thin_args(tensor4_args(draws, layout), thin), draws.ctypes.data_as(C.c_void_p), self.lib.mcr_sbc_ranks

    def sbc_ranks_rc(self, draws, truth, layout: str = "spcn", thin: int = 1) -> tuple[int, dict]:
        """sbc_ranks with the library's return code beside the result instead of an exception: MCR_ENONFINITE leaves the
        outputs written, a refusal leaves them as they were filled (-1 and NaN)."""
        targs, ptr, fn = self._sbc_call(draws, layout, thin)
        S, P = targs[1], targs[4]
        t = _truth_array(truth, S, P)
        arrs, out = _sbc_arrays(S, P)
        rc = fn(self.handle, ptr, *targs, _as_dp(t), C.byref(out))
        return rc, {**{k: a[:S, :P] for k, a in arrs.items()}, "n_draws": int(targs[2] * targs[3])}

    def sbc_ranks(self, draws, truth, layout: str = "spcn", thin: int = 1) -> dict:
        """Where every true value stands among its posterior draws, for S simulations at once (mcr_sbc_ranks: simulation-based
        calibration).  draws: a 4-D host array whose axes are `layout`, a permutation of "scnp" (strided views included), or a
        DeviceSims from upload_sims; truth [S][P].  thin = k takes the draws n = 0, k, 2k, ... of every chain.  [S][P]
        arrays: "n_less" and "n_equal" (int64: the draws below the truth, and equal to it), "mean", "sd" (population) of the
        L = C * ceil(N / k) pooled draws; and the int "n_draws" = L."""
        rc, res = self.sbc_ranks_rc(draws, truth, layout, thin)
        self._check(rc)
        return res

    def sbc_sims_per_chunk(self, draws, layout: str = "spcn", thin: int = 1) -> int:
        """Simulations per workspace chunk of an sbc_ranks call on these draws (mcr_sbc_plan); all S where the call reads
        the tensor in place."""
        return self._params_per_chunk("mcr_sbc_plan", self._sbc_call(draws, layout, thin)[0])

    def autocorr(self, draws, layout: str = "cnp", max_lag=None, unbiased: bool = False, window_c: float = 5.0) -> dict:
        """Autocorrelation functions and integrated autocorrelation times of the raw draws (mcr_autocorr: ArviZ's autocorr,
        emcee's integrated_time) of a host array (strided views included) or a DeviceTensor with equal-length chains.
        max_lag: the default is min(100, N - 1); at most MCR_ACF_MAX_LAG.  unbiased: divide lag l by N - l instead of N.
        Arrays: "acf" [P][C][L+1], "var" (gamma_0), "tau", "window" (int64, -1: the ACF has not decayed within max_lag and tau
        is a lower bound) and "ess_chain" = N / tau, all [P][C]; the within-chain pooled "acf_pooled" [P][L+1],
        "tau_pooled", "window_pooled", "ess_pooled" = C N / tau_pooled, all [P]; and the int "max_lag"."""
        targs, ptr, fn, _ = self._tensor_call(draws, layout, "autocorr", False)
        nc, N, P = targs[1], targs[2], targs[3]
        L = min(100, max(N - 1, 0)) if max_lag is None else int(max_lag)
        arrs, out = _acf_arrays(P, nc, L if 0 <= L <= MCR_ACF_MAX_LAG else 0)  # (a bad max_lag is refused before anything is written)
        self._check(fn(self.handle, ptr, *targs, L, MCR_ACF_UNBIASED if unbiased else 0, float(window_c), C.byref(out)))
        return _acf_result(arrs, P, nc, N, L)

    def autocorr_params_per_chunk(self, t: "DeviceTensor", max_lag: int) -> int:
        """Parameters per workspace chunk of an autocorr call with this max_lag on this tensor (mcr_autocorr_plan)."""
        return self._params_per_chunk("mcr_autocorr_plan", t, int(max_lag), call="autocorr")

    def covariance(self, draws) -> np.ndarray:
        """Population covariance (ddof=0) of draws [P][M] -> [P][P] (fp64 MFMA)."""
        x = np.ascontiguousarray(draws, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("draws must be 2-D [P][M]")
        P = x.shape[0]
        cov = np.full((max(P, 1), max(P, 1)), np.nan)
        self._check(self.lib.mcr_covariance(self.handle, _as_dp(x), x.shape[1], P, _as_dp(cov)))
        return cov[:P, :P] if P else np.empty((0, 0))
