"""Posterior diagnostics of a fitted VI_SSM: path and theta summaries, posterior-predictive forecasts, the particle
filters and the particle smoother.  PosteriorDiagnostics is a mixin of vi_ssm.VISSMBase: its methods reach the
model's engine, dist, mdef, p_local, global_step and target_len() directly, and none of them is part of training.

Every diagnostic summarises [rows, S * m] device chunks with summary.column_summary and lays the chunks' results
side by side over time (stack_bands); the save_* methods write the result as one .npz on rank 0 (_save_npz)."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .summary import DEFAULT_PROBS, _check_probs, column_summary

# Philox key of the forecast's normals: the engine's seed xor this (Engine.draw keys eps by the seed itself and the
# q(theta) base draw by seed ^ 0x5DEECE66D)
FORECAST_SEED_XOR = 0xF02ECA57
# Philox key of the particle filter's normals and resampling integers: a fourth key next to the forecast's
FILTER_SEED_XOR = 0xF117E2ED
# Philox key of the particle smoother's selection words: a fifth key
SMOOTH_SEED_XOR = 0x5300714E
# Philox key of the Metropolis-Hastings chains over theta (their filters' normals and resampling integers, their
# proposals and uniforms): a sixth key
MCMC_SEED_XOR = 0x3C3C7E7A
# filter steps one block runs per launch of theta_mcmc(): a launch holds max(1, MCMC_LAUNCH_STEPS // T) iterations.
# Measured at N = 1024 and 64 chains: 3.1 us per AR step, 0.81 s per launch at T = 5000;
# volatility_mcmc() (section 4.13): 4.3 us per SV step, 1.12 s per launch at T = 1508
MCMC_LAUNCH_STEPS = 1 << 18
# xor-ed into the chains' Philox key for the fresh carried normals of the correlated chain (ops.cpm_fresh_aux): their
# rows start at the iterations' base, under a key of their own
CPM_SEED_XOR = 0x436F72724E6F6973
# device bytes of the filter's cloud [K N, S, T] fp32 that particle_smoother() may keep for its backward pass
SMOOTH_CLOUD_BYTES = 8 << 30
# device bytes one forecast launch may write per output ([B, S, chunk] fp32): the default chunk is the largest
# multiple of the kernel's tile under it
FORECAST_CHUNK_BYTES = 256 << 20


def stack_bands(prefix: str, parts: List[Tuple[int, Dict[str, np.ndarray]]], S: int, Q: int) -> Dict[str, np.ndarray]:
    """{prefix}/{mean, sd, n_valid} [S, T] and {prefix}/quantiles [Q, S, T] from the chunks' column summaries in time
    order: parts = [(m, column_summary of a [rows, S * m] chunk)], coordinate-major within a chunk, T = sum of the m.
    No chunk: T = 0, float64 and (n_valid) int64 as otherwise."""
    res = {}
    for k, dt_ in (("mean", np.float64), ("sd", np.float64), ("n_valid", np.int64)):
        res[f"{prefix}/{k}"] = np.concatenate([s[k].reshape(S, m) for m, s in parts] +
                                              [np.zeros((S, 0), dtype=dt_)], axis=1)
    res[f"{prefix}/quantiles"] = np.concatenate([s["quantiles"].reshape(Q, S, m) for m, s in parts] +
                                                [np.zeros((Q, S, 0))], axis=2)
    return res


def split_rhat(x: np.ndarray) -> float:
    """Split-R-hat of draws x [C, n] (Gelman et al., BDA3 section 11.4): every chain cut into halves of m = n // 2 draws
    (the middle one of an odd n dropped), W the mean within-half variance, B = m var(half means):
    sqrt(((m - 1) / m W + B / m) / W).  NaN where W is 0 or a half has fewer than two draws."""
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[1] // 2
    if m < 2:
        return float("nan")
    h = np.concatenate([x[:, :m], x[:, x.shape[1] - m:]], axis=0)
    W = h.var(axis=1, ddof=1).mean()
    B = m * h.mean(axis=1).var(ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(((m - 1) / m * W + B / m) / W))


class PosteriorDiagnostics:
    """The diagnostics of VISSMBase (which sets filter_data = None and whose subclasses call _keep_filter_data)."""

    def _save_npz(self, PATH: str, res: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
        """res as one .npz, written by rank 0 only (every rank computed it)."""
        if self.dist.rank == 0:
            d = os.path.dirname(PATH)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(PATH, "wb") as f:
                np.savez(f, **res)
        return res

    def _chunk_steps(self, rows: int) -> int:
        """Steps per launch so that [rows, S, steps] fp32 stays under FORECAST_CHUNK_BYTES: a multiple of the
        forecast tile, at least one."""
        steps = FORECAST_CHUNK_BYTES // (4 * _lib.MODEL_S[self.mdef.model_id] * max(rows, 1))
        return max(_lib.SIM_TILE, steps // _lib.SIM_TILE * _lib.SIM_TILE)

    # ------------------------------------------------------------------ posterior summaries
    @torch.no_grad()
    def sample_paths_theta(self, starts: np.ndarray, step: int = 0):
        """sample_paths with the draw's theta next to the paths: (x [B, D, M+1], theta [B, P])."""
        batch = self.engine.make_batch(np.asarray(starts))
        out = self.forward(batch, step)
        return self.engine.lf_sample(out["z"], batch), out["theta"]

    @torch.no_grad()
    def posterior_summary(self, probs=DEFAULT_PROBS) -> Dict[str, np.ndarray]:
        """Mean, sd and quantile bands of the latent path over time and of theta, over exactly the samples save_paths
        would write (the same window starts, draws and step) and, with several ranks, over all of them -- computed on
        the GPU (summary.column_summary), so only the summaries reach the host instead of every sample of every
        window (AR.py:323-362 and the offline quantiles of vis.py).  paths/{mean, sd} are [D, T], paths/quantiles
        [Q, D, T]; theta/{mean, sd} [P], theta/quantiles [Q, P] come from the first window's draw, log-parameters
        exponentiated as in histograms().  Every rank takes part in the collectives and gets the same result."""
        M = self.batch_dims
        parts = []
        res: Dict[str, np.ndarray] = {"probs": np.asarray(list(probs), dtype=np.float64)}
        for idx in np.arange(0, self.target_len(), M):
            x, theta = self.sample_paths_theta(np.tile(idx, self.p_local), step=self.global_step)
            xs = x[:, :, 1:]
            B, D, m = xs.shape
            x2 = xs[:, 0, :] if D == 1 else xs.reshape(B, D * m)   # a pitched, offset view / a contiguous copy
            parts.append((m, column_summary(x2.float(), probs, self.dist)))
            if "theta/mean" not in res:
                th = theta.detach().float()
                pos = list(self.mdef.theta_pos)
                if any(pos):
                    th = torch.where(torch.tensor(pos, device=th.device), th.exp(), th)
                for k, v in column_summary(th.contiguous(), probs, self.dist).items():
                    res[f"theta/{k}"] = v
        res.update(stack_bands("paths", parts, D, res["probs"].size))
        return res

    def save_summary(self, PATH: str, probs=DEFAULT_PROBS) -> Dict[str, np.ndarray]:
        """posterior_summary written as one .npz by rank 0 (every rank computes it: the collectives need them all)."""
        return self._save_npz(PATH, self.posterior_summary(probs))

    # ------------------------------------------------------------------ posterior-predictive forecasts
    def forecast_chunk(self) -> int:
        """Steps per launch of forecast() by default: [p_local, S, chunk] fp32 stays under FORECAST_CHUNK_BYTES."""
        return self._chunk_steps(self.p_local)

    @torch.no_grad()
    def forecast(self, horizon: int, probs=DEFAULT_PROBS, obs: bool = False, chunk: Optional[int] = None
                 ) -> Dict[str, np.ndarray]:
        """Posterior-predictive forecast: the SDE simulated `horizon` steps past the data on the GPU
        (ops.sde_simulate), from every sample of the draw of the last window save_paths / posterior_summary visit
        (same start, same step) -- its theta and its path's last state -- and summarised over the samples of all
        ranks with summary.column_summary.  forecast/{mean, sd, n_valid} are [S, H], forecast/quantiles [Q, S, H]
        (S the state's coordinates; 2 for SV, the observed series and its log-volatility); obs=True adds the same
        four under forecast/obs/ for simulated observations x + obs_std * noise (not SV); forecast/start =
        target_len(), the index of the first forecast step.  A trajectory that leaves the model's domain is NaN
        from there on and n_valid counts the rest: the bands condition on survival.  The normals are
        Philox rows global_step * p + rank * p_local + b under key seed ^ FORECAST_SEED_XOR, so the result does not
        depend on the number of ranks; `chunk` steps per launch (default forecast_chunk()), chained through the end
        state, change nothing either.  Every rank takes part in the collectives and gets the same result."""
        from . import ops
        H = int(horizon)
        if H < 0:
            raise ValueError(f"forecast horizon {horizon} < 0")
        p = _check_probs(probs)
        md = self.mdef
        if obs and md.model_id == _lib.MODEL_SV:
            raise ValueError("forecast(obs=True): SV has no observation model (its first coordinate is the observed "
                             "series)")
        chunk = self.forecast_chunk() if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"forecast chunk {chunk} < 1")
        last = int(np.arange(0, self.target_len(), self.batch_dims)[-1])
        x, theta = self.sample_paths_theta(np.tile(last, self.p_local), step=self.global_step)
        th = theta.detach().float().contiguous()
        state = x[:, :, -1].float().contiguous()
        seed = self.engine.seed ^ FORECAST_SEED_XOR
        row0 = self.global_step * self.p + self.dist.rank * self.p_local
        S, Q = _lib.MODEL_S[md.model_id], p.size   # the state's coordinates (SV: 2; its mdef.D counts the latent one)
        groups = ("forecast", "forecast/obs") if obs else ("forecast",)
        parts = {g: [] for g in groups}
        for t0 in range(0, H, chunk):
            m = min(chunk, H - t0)
            xs, ys, state = ops.sde_simulate(md.model_id, th, state, m, md.dt, seed, row0, t0=t0,
                                             obs_std=md.obs_std if obs else None)
            for g, v in zip(groups, (xs, ys)):
                parts[g].append((m, column_summary(v.view(v.shape[0], S * m), probs, self.dist)))
        res: Dict[str, np.ndarray] = {"probs": p, "forecast/start": np.asarray(self.target_len(), dtype=np.int64)}
        for g in groups:
            res.update(stack_bands(g, parts[g], S, Q))
        return res

    def save_forecast(self, PATH: str, horizon: int, probs=DEFAULT_PROBS, obs: bool = False,
                      chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
        """forecast written as one .npz by rank 0 (every rank computes it: the collectives need them all)."""
        return self._save_npz(PATH, self.forecast(horizon, probs, obs, chunk))

    # ------------------------------------------------------------------ particle filter
    def filter_chunk(self, n_theta: int, n_particles: int) -> int:
        """Steps per launch of particle_filter() by default: the [K N, S, chunk] fp32 cloud stays under
        FORECAST_CHUNK_BYTES (a multiple of the forecast tile, at least one)."""
        return self._chunk_steps(n_theta * n_particles)

    @torch.no_grad()
    def particle_filter(self, n_theta: int = 64, n_particles: int = 1024, probs=DEFAULT_PROBS,
                        chunk: Optional[int] = None, proposal: str = "bootstrap") -> Dict[str, np.ndarray]:
        """A check of the fitted posterior that does not come out of the flows: K = n_theta bootstrap particle filters
        of N = n_particles particles each (ops.particle_filter), one per theta sample, over the model's observations
        from its x0.  theta = global samples 0 .. K - 1 of the first window's draw posterior_summary uses (same
        start, same step): rank 0's first rows, broadcast, so K <= p_local.  Every rank runs the identical
        deterministic launches and holds the same result; nothing is sharded.

        filter/loglik [K] float64 estimates log p(y | theta_k) (-inf: every particle died); filter/theta [K, P] the
        raw theta rows; filter/ll_inc and filter/ess [K, T] the per-step increments (0 where nothing is observed) and
        effective sample sizes (N there); filter/{mean, sd, n_valid} [S, T] and filter/quantiles [Q, S, T] summarise
        the K N equally weighted post-resampling particles of each step (summary.column_summary): the theta_k are iid
        from q(theta), so this is the filtering distribution averaged over q(theta).  T = min(target_len(), the
        observations' length).  Philox key seed ^ FILTER_SEED_XOR, rows global_step K N + k N + i; `chunk` steps per
        launch (default filter_chunk()), chained through the end state and the running log-likelihood, change
        nothing.  SV has no observation model: ValueError.

        proposal = "adapted" runs the fully adapted filter (ops.particle_filter(proposal="adapted")) on the same
        theta rows, key, rows and chunks: a much lower variance of filter/loglik where obs_std is small against the
        process noise.  The result then also carries filter/proposal = "adapted", and its bands summarise the
        post-propagation particles (n_valid leaves out the LV particles that left the orthant after a resampling).
        With the default every launch and every entry is the bootstrap filter's, with no new key.  Any other value:
        VissmError."""
        return self._filter_pass("particle_filter", n_theta, n_particles, None, probs, chunk, proposal)

    def _filter_pass(self, what, n_theta, n_particles, n_paths, probs, chunk, proposal):
        """particle_filter() and particle_smoother() (`what`; n_paths None for the filter): their own refusals, then
        _filter_smooth() on the model's observations from its x0 with ops.particle_filter / ops.particle_smooth."""
        from . import ops
        md = self.mdef
        if proposal not in ops.PF_PROPOSALS:
            raise _lib.VissmError(f"{what}: proposal {proposal!r}, one of {ops.PF_PROPOSALS} expected")
        if md.model_id == _lib.MODEL_SV or getattr(self, "filter_data", None) is None:
            raise ValueError(f"{what}: SV has no observation model (its first coordinate is the observed "
                             "series)")

        def data():
            dev = self.engine.device
            obs_h, bin_h, x0_h = self.filter_data
            T = min(int(self.target_len()), obs_h.shape[1])
            obs = torch.as_tensor(np.ascontiguousarray(obs_h[:, :T]), device=dev)
            obs_bin = torch.as_tensor(np.ascontiguousarray(bin_h[:, :T]), device=dev)
            step = lambda th, state, N, seed, row0, **kw: ops.particle_filter(
                md.model_id, th, state, obs, obs_bin, md.dt, md.obs_std, N, seed, row0, cloud=True, proposal=proposal,
                **kw)
            smooth = lambda th, cloud, M, seed, row0, **kw: ops.particle_smooth(md.model_id, th, cloud, md.dt, M, seed,
                                                                                row0, **kw)
            return T, torch.as_tensor(x0_h, device=dev), step, smooth

        # the sizes' refusals carry particle_filter's name for the smoother too
        return self._filter_smooth(what, "particle_filter", _lib.MODEL_S[md.model_id], data, n_theta, n_particles,
                                   n_paths, probs, chunk, proposal)

    def _broadcast_rank0(self, t: torch.Tensor) -> torch.Tensor:
        """t overwritten on every rank with rank 0's (one process: t as it is)."""
        if self.dist.world > 1:
            import torch.distributed as dist
            dist.broadcast(t, src=dist.get_global_rank(self.dist.group, 0) if self.dist.group is not None else 0,
                           group=self.dist.group)
        return t

    def _filter_smooth(self, what, label, S, data, n_theta, n_particles, n_paths, probs, chunk, proposal):
        """The launches and the result of the two filters (n_paths None) and the two smoothers, for the public method
        `what`; `label` is the name its refusals of n_particles, n_theta and chunk carry, S the filtered state's
        coordinates, proposal what filter/proposal reports ("bootstrap": no such entry).  data(), called once those
        sizes are checked, raises the refusals of the data and returns (T, state, step, smooth): the steps, the start
        state and the two ops calls, step(th, state, N, seed, row0, t0=, loglik_in=, H=) and smooth(th, cloud, M, seed,
        row0, t0=, x_next=).  A smoother's n_paths, T and cloud bytes are checked before the first launch, and every
        chunk's cloud then stays on the device until the backward pass has smoothed it."""
        K, N = int(n_theta), int(n_particles)
        if N not in _lib.PF_PARTICLES:
            raise ValueError(f"{label}: n_particles={N}, one of {_lib.PF_PARTICLES} expected")
        if not 1 <= K <= self.p_local:
            raise ValueError(f"{label}: n_theta={K} outside 1 .. p_local = {self.p_local}")
        p = _check_probs(probs)
        chunk = self.filter_chunk(K, N) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"{label} chunk {chunk} < 1")
        T, state, step, smooth = data()
        if n_paths is not None:
            M, cap = int(n_paths), SMOOTH_CLOUD_BYTES
            if not (_lib.PS_MIN_PATHS <= M <= N and M & (M - 1) == 0):
                raise ValueError(f"{what}: n_paths={M}, a power of two in {_lib.PS_MIN_PATHS} .. n_particles = {N} "
                                 "expected")
            if T < 1:
                raise ValueError(f"{what}: no step to smooth")
            if 4 * K * N * S * T > cap:
                raise ValueError(f"{what}: the filter's cloud [{K} * {N}, {S}, {T}] fp32 takes {4 * K * N * S * T} "
                                 f"bytes, more than SMOOTH_CLOUD_BYTES = {cap}: lower n_theta or n_particles")
        dev = self.engine.device
        Q = p.size
        _, theta = self.sample_paths_theta(np.tile(0, self.p_local), step=self.global_step)
        th = self._broadcast_rank0(theta.detach().float()[:K].contiguous())
        row0 = self.global_step * K * N
        ll = None
        incs, esss, parts, clouds = [], [], [], []
        for t0 in range(0, T, chunk):
            m = min(chunk, T - t0)
            r = step(th, state, N, self.engine.seed ^ FILTER_SEED_XOR, row0, t0=t0, loglik_in=ll, H=m)
            state, ll = r.state_end, r.loglik
            incs.append(r.ll_inc)
            esss.append(r.ess)
            parts.append((m, column_summary(r.cloud.view(K * N, S * m), probs, None)))
            if n_paths is not None:
                clouds.append((t0, r.cloud))
        res: Dict[str, np.ndarray] = {"probs": p, "filter/theta": th.cpu().numpy()}
        if proposal != "bootstrap":
            res["filter/proposal"] = np.asarray(proposal)
        res["filter/loglik"] = ll.cpu().numpy() if ll is not None else np.zeros(K)
        res["filter/ll_inc"] = torch.cat(incs + [torch.zeros(K, 0, device=dev)], 1).cpu().numpy()
        res["filter/ess"] = torch.cat(esss + [torch.zeros(K, 0, device=dev)], 1).cpu().numpy()
        res.update(stack_bands("filter", parts, S, Q))
        parts, x_next = [], None
        while clouds:
            t0, cloud = clouds.pop()          # last chunk first; the cloud is freed once it is smoothed
            r = smooth(th, cloud, M, self.engine.seed ^ SMOOTH_SEED_XOR, row0, t0=t0, x_next=x_next)
            x_next = r.x_first
            m = cloud.shape[2]
            parts.append((m, column_summary(r.paths.view(K * M, S * m), probs, None)))
            del cloud, r
        if n_paths is not None:
            res.update(stack_bands("smooth", parts[::-1], S, Q))
        return res

    def save_filter(self, PATH: str, n_theta: int = 64, n_particles: int = 1024, probs=DEFAULT_PROBS,
                    chunk: Optional[int] = None, proposal: str = "bootstrap") -> Dict[str, np.ndarray]:
        """particle_filter written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.particle_filter(n_theta, n_particles, probs, chunk, proposal))

    # ------------------------------------------------------------------ the theta posterior by PMMH
    @torch.no_grad()
    def theta_mcmc(self, n_chains: int = 64, n_particles: int = 256, n_iter: int = 2000, burn_in: int = 500,
                   step_scale: float = 1.0, probs=DEFAULT_PROBS, adapt: bool = False, target_accept: float = 0.234,
                   adapt_decay: float = 0.5, correlation: float = 0.0) -> Dict[str, np.ndarray]:
        """The posterior p(theta | y) to lay over q(theta): C = n_chains particle marginal Metropolis-Hastings chains
        (ops.pmmh; Andrieu, Doucet & Holenstein 2010) whose acceptance ratio holds the fully adapted filter's unbiased
        estimate of p(y | theta) from N = n_particles particles, so they target p(theta | y) exactly for any N.  The
        prior is the model's (mdef.priors, independent Gaussians on the raw theta), the data and x0 the filter's.

        The random walk's covariance is step_scale^2 (2.38^2 / P) Sigma_q with Sigma_q the float64 sample covariance
        of the raw theta draw posterior_summary uses (rank 0's rows, broadcast); ValueError if it is not positive
        definite (a q(theta) much wider than the posterior makes that walk too wide and nearly every proposal is
        rejected: lower step_scale; mcmc/accept_rate and mcmc/rhat show it).  Chain c starts at sample c of that draw (C <= p_local) with the estimate of
        ops.particle_filter(proposal="adapted", cloud=False).  The run is cut into launches of
        max(1, MCMC_LAUNCH_STEPS // T) iterations chained through theta_end / ll_end, which changes nothing.  Philox
        key seed ^ MCMC_SEED_XOR, rows based at global_step C N (n_iter + 1): the initial filters take the first C N
        rows, iteration i the next.  Every rank runs the identical launches and holds the same result.

        mcmc/theta [C, n_keep, P] (raw) and mcmc/loglik [C, n_keep] are the draws after burn_in; mcmc/accept_rate [C];
        mcmc/{mean, sd} [P] and mcmc/quantiles [Q, P] summarise the pooled draws on theta/quantiles' scale
        (log-parameters exponentiated) at the same probs and by the same estimator, with theta/{mean, sd, quantiles}
        of q(theta) copied in beside them; mcmc/rhat [P] is the split-R-hat of the raw draws; mcmc/prop_chol [P, P].
        SV has no observation model: ValueError (volatility_mcmc() is SV's).

        adapt = True: one fixed factor shared by all chains mixes badly when q(theta) is much wider than the posterior
        in some coordinate (a few per mille accepted).  Then every chain starts from that factor and adapts its own
        over the iterations [0, burn_in) inside the kernel (ops.pmmh_adaptive: robust adaptive Metropolis, a rank-one
        update of the factor after every decision, steered to the acceptance rate target_accept with step sizes
        min(1, P (i + 1)^-adapt_decay)), and keeps it frozen after: the kept draws come from an ordinary fixed-proposal
        chain, which targets p(theta | y) exactly.  The launches are cut as before and chained through chol_end as
        well.  The result gains mcmc/prop_chol_end [C, P, P], the chains' frozen factors, and mcmc/accept_rate_adapt
        [C], the acceptance over the adaptation; mcmc/prop_chol stays the starting factor.  burn_in = 0,
        target_accept outside (0, 1) or adapt_decay outside (0, 1]: ValueError.  With adapt = False nothing changes.

        correlation: the correlated pseudo-marginal chain is built for SV only (volatility_mcmc(); a one-dimensional
        state sorts by value, LV and FHN would need a space-filling order): anything but 0.0 is a ValueError."""
        from . import ops
        md = self.mdef
        if float(correlation) != 0.0:
            raise ValueError(f"theta_mcmc: correlation={correlation}: the correlated chain is not built for AR, LV and "
                             "FHN (volatility_mcmc() has it for SV)")
        if md.model_id == _lib.MODEL_SV or getattr(self, "filter_data", None) is None:
            raise ValueError("theta_mcmc: SV has no observation model (its first coordinate is the observed series)")
        C, N, n_iter, burn, p = self._mcmc_args("theta_mcmc", n_chains, n_particles, n_iter, burn_in, step_scale, probs)
        if adapt:
            target_accept, adapt_decay = self._mcmc_adapt_args("theta_mcmc", burn, target_accept, adapt_decay)
        dev = self.engine.device
        P = _lib.MODEL_P[md.model_id]
        obs_h, bin_h, x0_h = self.filter_data
        T = min(int(self.target_len()), obs_h.shape[1])
        obs = torch.as_tensor(np.ascontiguousarray(obs_h[:, :T]), device=dev)
        obs_bin = torch.as_tensor(np.ascontiguousarray(bin_h[:, :T]), device=dev)
        x0 = torch.as_tensor(np.asarray(x0_h, dtype=np.float32).reshape(-1), device=dev)
        draw, chol, L, prior = self._mcmc_walk("theta_mcmc", P, step_scale)
        seed = self.engine.seed ^ MCMC_SEED_XOR
        row0 = self.global_step * C * N * (n_iter + 1)
        th = draw[:C].contiguous()
        ll = ops.particle_filter(md.model_id, th, x0, obs, obs_bin, md.dt, md.obs_std, N, seed, row0, cloud=False,
                                 proposal="adapted").loglik
        if adapt:
            def step(it0, n, th, ll, Lc):
                r = ops.pmmh_adaptive(md.model_id, th, ll, Lc, prior, x0, obs, obs_bin, md.dt, md.obs_std, N, n, seed,
                                      row0 + C * N, burn, target_accept, adapt_decay, it0=it0)
                return r, (r.theta_end, r.ll_end, r.chol_end)
        else:
            def step(it0, n, th, ll):
                r = ops.pmmh(md.model_id, th, ll, L, prior, x0, obs, obs_bin, md.dt, md.obs_std, N, n, seed,
                             row0 + C * N, it0=it0)
                return r, (r.theta_end, r.ll_end)
        runs, end = self._mcmc_launches(n_iter, T, (th, ll) + ((L.repeat(C, 1, 1),) if adapt else ()), step)
        return self._mcmc_result(runs, burn, p, probs, chol, draw, end[2] if adapt else None)

    @staticmethod
    def _mcmc_launches(n_iter, T, state, step):
        """The run of theta_mcmc() / volatility_mcmc() cut into launches of max(1, MCMC_LAUNCH_STEPS // T) iterations:
        step(it0, n, *state) runs iterations it0 .. it0 + n - 1 and returns (its result, the state the next launch
        takes: theta_end, ll_end and, where the chains carry their factors, chol_end).  ([results], the last state)."""
        per = max(1, MCMC_LAUNCH_STEPS // max(T, 1))
        runs = []
        for it0 in range(0, n_iter, per):
            r, state = step(it0, min(per, n_iter - it0), *state)
            runs.append(r)
        return runs, state

    def _mcmc_args(self, what, n_chains, n_particles, n_iter, burn_in, step_scale, probs):
        """The checks theta_mcmc() and volatility_mcmc() share: (C, N, n_iter, burn, p)."""
        C, N, n_iter, burn = int(n_chains), int(n_particles), int(n_iter), int(burn_in)
        if N not in _lib.PF_PARTICLES:
            raise ValueError(f"{what}: n_particles={N}, one of {_lib.PF_PARTICLES} expected")
        if not 1 <= C <= self.p_local:
            raise ValueError(f"{what}: n_chains={C} outside 1 .. p_local = {self.p_local}")
        if not 0 <= burn < n_iter:
            raise ValueError(f"{what}: burn_in={burn} outside 0 .. n_iter - 1 = {n_iter - 1}")
        if not 0.0 < float(step_scale) < float("inf"):
            raise ValueError(f"{what}: step_scale={step_scale} must be positive and finite")
        return C, N, n_iter, burn, _check_probs(probs)

    @staticmethod
    def _mcmc_adapt_args(what, burn, target_accept, adapt_decay):
        """The checks adapt = True adds: (target_accept, adapt_decay)."""
        target_accept, adapt_decay = float(target_accept), float(adapt_decay)
        if burn < 1:
            raise ValueError(f"{what}: adapt=True adapts over the iterations [0, burn_in): burn_in={burn} leaves none")
        if not 0.0 < target_accept < 1.0:
            raise ValueError(f"{what}: target_accept={target_accept} outside (0, 1)")
        if not 0.0 < adapt_decay <= 1.0:
            raise ValueError(f"{what}: adapt_decay={adapt_decay} outside (0, 1]")
        return target_accept, adapt_decay

    def _mcmc_walk(self, what, P, step_scale):
        """The raw theta draw posterior_summary uses (rank 0's rows, broadcast), the factor of the random walk's
        covariance step_scale^2 (2.38^2 / P) Sigma_q in float64 and as the fp32 device tensor the kernel takes, and
        the model's prior [P, 2]: (draw, chol, L, prior)."""
        dev = self.engine.device
        _, theta = self.sample_paths_theta(np.tile(0, self.p_local), step=self.global_step)
        draw = self._broadcast_rank0(theta.detach().float().contiguous())
        sigma = np.atleast_2d(np.cov(draw.cpu().numpy().astype(np.float64).T))
        try:
            if not np.isfinite(sigma).all():
                raise np.linalg.LinAlgError
            chol = np.linalg.cholesky(float(step_scale) ** 2 * (2.38 ** 2 / P) * sigma)
        except np.linalg.LinAlgError:
            raise ValueError(f"{what}: the sample covariance of q(theta) is not positive definite") from None
        L = torch.as_tensor(chol.astype(np.float32), device=dev)
        prior = torch.as_tensor(np.asarray(self.mdef.priors, dtype=np.float32).reshape(P, 2), device=dev)
        return draw, chol, L, prior

    def _mcmc_result(self, runs, burn, p, probs, chol, draw, chol_end=None) -> Dict[str, np.ndarray]:
        """The result of theta_mcmc() / volatility_mcmc() from the chained launches' PmmhResults; chol_end: the
        adaptive chains' frozen factors (adapt = True), which adds mcmc/prop_chol_end and mcmc/accept_rate_adapt."""
        md, dev = self.mdef, self.engine.device
        P = _lib.MODEL_P[md.model_id]
        kept = torch.cat([r.theta_chain for r in runs], 1)[:, burn:].contiguous()
        res: Dict[str, np.ndarray] = {"probs": p, "mcmc/theta": kept.cpu().numpy(),
                                      "mcmc/loglik": torch.cat([r.ll_chain for r in runs], 1)[:, burn:].cpu().numpy(),
                                      "mcmc/accept_rate": torch.cat([r.accept for r in runs], 1)[:, burn:].double()
                                      .mean(1).cpu().numpy(),
                                      "mcmc/prop_chol": chol}
        if chol_end is not None:
            res["mcmc/prop_chol_end"] = chol_end.cpu().numpy()
            res["mcmc/accept_rate_adapt"] = torch.cat([r.accept for r in runs], 1)[:, :burn].double().mean(1).cpu().numpy()
        pooled = kept.view(-1, P)
        pos = list(md.theta_pos)
        if any(pos):
            pooled = torch.where(torch.tensor(pos, device=dev), pooled.exp(), pooled)
        for k, v in column_summary(pooled.contiguous(), probs, None).items():
            if k != "n_valid":
                res[f"mcmc/{k}"] = v
        res["mcmc/rhat"] = np.array([split_rhat(res["mcmc/theta"][:, :, i]) for i in range(P)])
        qd = draw
        if any(pos):
            qd = torch.where(torch.tensor(pos, device=dev), qd.exp(), qd)
        for k, v in column_summary(qd.contiguous(), probs, None).items():
            if k != "n_valid":
                res[f"theta/{k}"] = v
        return res

    def save_theta_mcmc(self, PATH: str, n_chains: int = 64, n_particles: int = 256, n_iter: int = 2000,
                        burn_in: int = 500, step_scale: float = 1.0, probs=DEFAULT_PROBS, adapt: bool = False,
                        target_accept: float = 0.234, adapt_decay: float = 0.5,
                        correlation: float = 0.0) -> Dict[str, np.ndarray]:
        """theta_mcmc written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.theta_mcmc(n_chains, n_particles, n_iter, burn_in, step_scale, probs, adapt,
                                                    target_accept, adapt_decay, correlation))

    # ------------------------------------------------------------------ the theta posterior of the SV family
    @torch.no_grad()
    def volatility_mcmc(self, n_chains: int = 64, n_particles: int = 256, n_iter: int = 2000, burn_in: int = 500,
                        step_scale: float = 1.0, probs=DEFAULT_PROBS, adapt: bool = False,
                        target_accept: float = 0.234, adapt_decay: float = 0.5,
                        correlation: float = 0.0) -> Dict[str, np.ndarray]:
        """theta_mcmc() for the SV family, which theta_mcmc() refuses: the same chains (ops.sv_pmmh) around
        volatility_filter()'s filter, which is exactly fully adapted.  The data and its refusals are that method's: the
        observed series y[0 .. T], every particle started at x0; ValueError for a family other than SV, a y[0 .. T]
        that is not finite, a y[0 .. T - 1] equal to 0.  The prior, the random walk's covariance step_scale^2 (2.38^2 /
        4) Sigma_q, the start at samples 0 .. C - 1 of the broadcast draw, the Philox key seed ^ MCMC_SEED_XOR, the rows
        based at global_step C N (n_iter + 1) (the initial estimates, ops.sv_filter(cloud=False), take the first C N),
        the launches of max(1, MCMC_LAUNCH_STEPS // T) iterations and every returned key are theta_mcmc()'s, and so
        are adapt, target_accept and adapt_decay (ops.sv_pmmh_adaptive) with the two keys they add.

        correlation = rho in (0, 0.9999]: the correlated pseudo-marginal chain (ops.sv_cpmmh; Deligiannidis, Doucet &
        Pitt 2018).  Each chain carries its filter's normals (ops.cpm_fresh_aux under the key seed ^ MCMC_SEED_XOR ^
        CPM_SEED_XOR, rows from the same base), proposes them by u' = rho u + sqrt(1 - rho^2) eps and resamples in
        sorted order (ops.sv_filter_sorted gives the initial estimates), which takes most of the estimate's noise out of
        the acceptance ratio at the same N; the chain still targets p(theta | y) exactly.  The launches are cut as
        before, the carried normals persisting across them; adapt composes.  The result gains mcmc/correlation.  0.0
        takes the path above unchanged; anything else is a ValueError."""
        from . import ops
        md = self.mdef
        rho = float(correlation)
        if not 0.0 <= rho <= 0.9999:
            raise ValueError(f"volatility_mcmc: correlation={correlation} outside [0, 0.9999]")
        if md.model_id != _lib.MODEL_SV:
            raise ValueError(f"volatility_mcmc: the {md.family} family has an observation model: theta_mcmc() is its "
                             "check; this one is SV's")
        C, N, n_iter, burn, p = self._mcmc_args("volatility_mcmc", n_chains, n_particles, n_iter, burn_in, step_scale,
                                                probs)
        if adapt:
            target_accept, adapt_decay = self._mcmc_adapt_args("volatility_mcmc", burn, target_accept, adapt_decay)
        y_h, T = self._volatility_series("volatility_mcmc")
        dev = self.engine.device
        P = _lib.MODEL_P[md.model_id]
        obs = torch.as_tensor(y_h, device=dev)
        h0 = torch.full((1,), float(self.x0), dtype=torch.float32, device=dev)
        draw, chol, L, prior = self._mcmc_walk("volatility_mcmc", P, step_scale)
        seed = self.engine.seed ^ MCMC_SEED_XOR
        row0 = self.global_step * C * N * (n_iter + 1)
        th = draw[:C].contiguous()
        if rho > 0.0:
            aux_n, aux_r, aux_sel = ops.cpm_fresh_aux(C, T, N, seed ^ CPM_SEED_XOR, row0, dev)
            ll = ops.sv_filter_sorted(th, h0, obs, md.dt, N, aux_n[:, 0].contiguous(),
                                      aux_r[:, 0].contiguous()).loglik

            def step(it0, n, th, ll, Lc):
                r = ops.sv_cpmmh(th, ll, Lc, prior, h0, obs, md.dt, N, n, seed, row0 + C * N, rho, aux_n, aux_r,
                                 aux_sel, burn if adapt else 0, target_accept, adapt_decay, it0=it0)
                return r, (r.theta_end, r.ll_end, r.chol_end)
        else:
            ll = ops.sv_filter(th, h0, obs, md.dt, N, seed, row0, cloud=False).loglik
            if adapt:
                def step(it0, n, th, ll, Lc):
                    r = ops.sv_pmmh_adaptive(th, ll, Lc, prior, h0, obs, md.dt, N, n, seed, row0 + C * N, burn,
                                             target_accept, adapt_decay, it0=it0)
                    return r, (r.theta_end, r.ll_end, r.chol_end)
            else:
                def step(it0, n, th, ll):
                    r = ops.sv_pmmh(th, ll, L, prior, h0, obs, md.dt, N, n, seed, row0 + C * N, it0=it0)
                    return r, (r.theta_end, r.ll_end)
        carried = rho > 0.0 or adapt                 # these chains hold a factor each
        runs, end = self._mcmc_launches(n_iter, T, (th, ll) + ((L.repeat(C, 1, 1),) if carried else ()), step)
        res = self._mcmc_result(runs, burn, p, probs, chol, draw, end[2] if adapt else None)
        if rho > 0.0:
            res["mcmc/correlation"] = np.float64(rho)
        return res

    def save_volatility_mcmc(self, PATH: str, n_chains: int = 64, n_particles: int = 256, n_iter: int = 2000,
                             burn_in: int = 500, step_scale: float = 1.0, probs=DEFAULT_PROBS, adapt: bool = False,
                             target_accept: float = 0.234, adapt_decay: float = 0.5,
                             correlation: float = 0.0) -> Dict[str, np.ndarray]:
        """volatility_mcmc written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.volatility_mcmc(n_chains, n_particles, n_iter, burn_in, step_scale, probs,
                                                         adapt, target_accept, adapt_decay, correlation))

    # ------------------------------------------------------------------ particle smoother
    @torch.no_grad()
    def particle_smoother(self, n_theta: int = 64, n_particles: int = 1024, n_paths: int = 64, probs=DEFAULT_PROBS,
                          chunk: Optional[int] = None, proposal: str = "bootstrap") -> Dict[str, np.ndarray]:
        """The check that is comparable with what the engine fits: the variational posterior over the latent path is
        a smoothing distribution p(x_t | y_1:T), the filter's bands are filtering distributions p(x_t | y_1:t).
        Forward filtering, then backward simulation (ops.particle_smooth): the forward pass is particle_filter()'s,
        launch for launch (same theta rows, key, rows and chunks), with every chunk's cloud kept on the device --
        4 K N S T bytes, refused with ValueError before any launch above SMOOTH_CLOUD_BYTES; then M = n_paths
        trajectories per filter (a power of two, 64 <= M <= N) are drawn backward through the chunks, last to first,
        each chunk's first state the target of the one before, under the key seed ^ SMOOTH_SEED_XOR and rows
        global_step K N + k N + j.

        Returns every filter/* entry of particle_filter() plus smooth/{mean, sd, n_valid} [S, T] and
        smooth/quantiles [Q, S, T], the column summary of the K M trajectories of each step: the smoothing
        distribution averaged over q(theta), to lay over paths/quantiles of posterior_summary().  A filter that died
        contributes NaN trajectories, which n_valid leaves out.  `chunk` changes nothing; every rank runs the same
        launches and holds the same result.  SV has no observation model: ValueError.

        proposal = "adapted": the forward pass is particle_filter(proposal="adapted")'s, whose cloud is, like the
        bootstrap's, an equally weighted sample of each filtering law; the backward pass is untouched."""
        return self._filter_pass("particle_smoother", n_theta, n_particles, int(n_paths), probs, chunk, proposal)

    def save_smoother(self, PATH: str, n_theta: int = 64, n_particles: int = 1024, n_paths: int = 64,
                      probs=DEFAULT_PROBS, chunk: Optional[int] = None,
                      proposal: str = "bootstrap") -> Dict[str, np.ndarray]:
        """particle_smoother written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.particle_smoother(n_theta, n_particles, n_paths, probs, chunk, proposal))

    # ------------------------------------------------------------------ stochastic volatility: filter and smoother
    @torch.no_grad()
    def volatility_filter(self, n_theta: int = 64, n_particles: int = 1024, probs=DEFAULT_PROBS,
                          chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
        """particle_filter() for the SV family, which that method refuses: SV has no obs_std / obs_bin observation
        model, but its observed series y is the first coordinate of the state and the latent log-volatility h the
        second, so h can be filtered on p(y_t+1 | y_t, h_t) (ops.sv_filter).  The weight depends on the pre-step
        state and the move does not depend on y, so this is the exactly fully adapted filter, at no extra cost.

        K = n_theta filters of N = n_particles particles, one per theta sample, from h_0 = the model's x0 over y =
        the model's obs; theta rows, key (seed ^ FILTER_SEED_XOR), rows (global_step K N + k N + i), chunks and
        chaining as particle_filter().  The result has particle_filter()'s keys with S = 1 and T = target_len(), and
        filter/proposal = "adapted": filter/loglik [K] estimates log p(y_1:T | y_0, h_0, theta_k); column t of
        filter/{mean, sd, n_valid, quantiles} summarises the K N equally weighted particles of p(h_t+1 | y_0:t+1).
        ValueError before any launch: a family other than SV, a y[0 .. T] that is not finite, a y[0 .. T - 1] equal
        to 0 (the density degenerates)."""
        return self._volatility_pass("volatility_filter", n_theta, n_particles, None, probs, chunk)

    def _volatility_pass(self, what, n_theta, n_particles, n_paths, probs, chunk):
        """volatility_filter() and volatility_smoother() (`what`; n_paths None for the filter): their own refusal, then
        _filter_smooth() on the observed series from h_0 = x0 with ops.sv_filter / ops.sv_smooth."""
        from . import ops
        md = self.mdef
        if md.model_id != _lib.MODEL_SV:
            raise ValueError(f"{what}: the {md.family} family has an observation model: particle_filter() and "
                             "particle_smoother() are its checks; this one is SV's")

        def data():
            y_h, T = self._volatility_series(what)
            dev = self.engine.device
            obs = torch.as_tensor(y_h, device=dev)
            step = lambda th, state, N, seed, row0, **kw: ops.sv_filter(th, state, obs, md.dt, N, seed, row0,
                                                                        cloud=True, **kw)
            smooth = lambda th, cloud, M, seed, row0, **kw: ops.sv_smooth(th, cloud, obs, md.dt, M, seed, row0, **kw)
            return T, torch.full((1,), float(self.x0), dtype=torch.float32, device=dev), step, smooth

        return self._filter_smooth(what, what, 1, data, n_theta, n_particles, n_paths, probs, chunk, "adapted")

    def _volatility_series(self, what):
        """The observed series y[0 .. T] fp32 the SV filter reads and T, refused where it is not finite or a y[0 .. T - 1]
        is 0."""
        y_h = np.asarray(self.obs, dtype=np.float32).reshape(-1)
        T = min(int(self.target_len()), y_h.shape[0] - 1)
        y_h = np.ascontiguousarray(y_h[:T + 1])
        if not np.isfinite(y_h).all():
            raise ValueError(f"{what}: the observed series y[0 .. {T}] is not finite")
        if np.any(y_h[:T] == 0.0):
            raise ValueError(f"{what}: y[{int(np.flatnonzero(y_h[:T] == 0.0)[0])}] = 0: the density of the next "
                             "observation degenerates there")
        return y_h, T

    def save_volatility_filter(self, PATH: str, n_theta: int = 64, n_particles: int = 1024, probs=DEFAULT_PROBS,
                               chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
        """volatility_filter written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.volatility_filter(n_theta, n_particles, probs, chunk))

    @torch.no_grad()
    def volatility_smoother(self, n_theta: int = 64, n_particles: int = 1024, n_paths: int = 64, probs=DEFAULT_PROBS,
                            chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
        """particle_smoother() for the SV family: volatility_filter()'s forward pass, launch for launch, with every
        chunk's cloud kept on the device (4 K N T bytes, refused above SMOOTH_CLOUD_BYTES), then M = n_paths
        trajectories of h per filter drawn backward through the chunks (ops.sv_smooth) under the key seed ^
        SMOOTH_SEED_XOR and rows global_step K N + k N + j.  Returns every filter/* entry plus smooth/{mean, sd,
        n_valid} [1, T] and smooth/quantiles [Q, 1, T]: column t is p(h_t+1 | y_0:T) averaged over q(theta), to lay
        directly over paths/quantiles of posterior_summary().  `chunk` changes nothing; every rank runs the same
        launches and holds the same result.  Refusals as volatility_filter()."""
        return self._volatility_pass("volatility_smoother", n_theta, n_particles, int(n_paths), probs, chunk)

    def save_volatility_smoother(self, PATH: str, n_theta: int = 64, n_particles: int = 1024, n_paths: int = 64,
                                 probs=DEFAULT_PROBS, chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
        """volatility_smoother written as one .npz by rank 0 (every rank computes the same result)."""
        return self._save_npz(PATH, self.volatility_smoother(n_theta, n_particles, n_paths, probs, chunk))

    def _keep_filter_data(self, obs, obs_bin, x0):
        """The raw constructor arguments the particle filter reads (the feature tables are built from copies):
        obs, obs_bin as [S, T] fp32, x0 as [S] fp32."""
        S = _lib.MODEL_S[self.mdef.model_id]
        self.filter_data = (np.asarray(obs, dtype=np.float32).reshape(S, -1),
                            np.asarray(obs_bin, dtype=np.float32).reshape(S, -1),
                            np.asarray(x0, dtype=np.float32).reshape(S))
