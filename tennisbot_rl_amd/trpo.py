"""TRPO on the batched envs: the trust-region policy step as HIP kernels (csrc/tb_trpo.hpp; C ABI tb_trpo_fvp / tb_trpo_search
in include/tb_stepper.h), the collect, GAE and critic of the PPO trainer around it.

`TRPOTrainer` collects exactly as `PPOTrainer` does (fused rollout, tb_ppo_gae) and has the same critic. `FusedTRPO.update`
replaces the policy's minibatch epochs with ONE step whose structure and constants are the reference's agent.py (TRPOAgent):

  1. g = grad_theta mean(ratio * A_hat), the surrogate of agent.py:99-107. theta = log_std, policy_net, action_net (the LOG_STD, PI
     and PI_HEAD slots of the flat vector); A_hat = the rollout's advantages normalised over the whole batch (mean, unbiased
     std + 1e-8). tb_ppo_grad computes exactly -g when its clip never binds (clip_range = inf), so it is reused unchanged.
  2. Fisher-vector products on cg_state_percent = 0.1 of the rows, drawn by one torch.randperm (agent.py:18,218-220):
     F v = (1/m) sum_rows J^T diag(sigma^-2) J v on the network's slots, 2 v on log_std, plus cg_damping * v (0.001). That is the
     Hessian of KL(old || new) at theta, which agent.py:144-167 obtains by double backprop.
  3. Conjugate gradient, agent.py:169-191: 10 iterations, x, r and the scalars in float64, p in float32; torch vector ops.
  4. beta = sqrt(2 delta / (x^T F x)), delta = kl_delta = 0.01 (agent.py:110-111).
  5. Line search: theta_k = theta + beta 1.5^-k x, k = 0 .. 9 (agent.py:112-113), all ten in one launch over all rows; the first
     k whose L_k = mean(ratio_k A_hat) and KL_k (agent.py:92-97) are finite with KL_k <= delta and L_k >= 0 (agent.py:132) is
     taken; if none qualifies theta stays as it is, bit for bit. The choice is made on the device.
  6. The critic: n_epochs passes of minibatch Adam on the value loss alone (tb_ppo_apply with TB_PPO_VALUE_ONLY): the policy
     slots of the parameters, the gradient and both Adam moments are not written.

Deviations of form="agent" from agent.py, all of them (form="agent_returns", below, lifts the first, the third, the fourth and the fifth):
  * log_std is inside the natural gradient (its Fisher block is 2 I); agent.py:120,136 moves it by the raw gradient
    (log_std_step="raw" does that in any form).
  * CG's early exit at rdotr < 1e-10 (agent.py:189-190) is a device-side freeze (torch.where): nothing synchronises.
  * x^T F x of the step size is taken over the CG rows, not over all rows (agent.py:110-111 uses all; step_rows="all" does in any form).
  * agent.py has no critic: it weights by normalised discounted returns (agent.py:210,264-268). Here GAE and a critic, as
    `-s trpo` of train_swing.py (a learner with a value function) implies.
  * log_std starts at 0, build_actor_critic's; agent.py:39-42 starts it at exp(-1) (log_std_init sets it in any form).
  * The ratio's old log-probability is the rollout's own (as in the PPO learner), and the CG rows are the first 0.1 n entries of
    a device-side torch.randperm instead of numpy's choice.

An update issues no host synchronisation before its single read of the statistics. One rank only, and only the architectures
the kernels are instantiated for: the env's default net_arch, or policy="mlp64" (NET_MLP64: SB3's [64, 64] on SwingRacket-v0).
There is no torch fallback: a refused call raises, as in learner.py.

form="sb3": sb3_contrib's TRPO, what the reference's `train_swing.py -s trpo` runs (train_swing.py:101-102, `TRPO("MlpPolicy", env)`).
The same six steps on the same kernels with sb3_contrib's constants (SB3_TRPO_DEFAULTS) and its acceptance rule:
  2'. every row takes part in the Fisher-vector products (cg_state_percent = 1.0: sub_sampling_factor = 1), cg_damping = 0.1.
  3'. 15 CG iterations.
  4'. beta = sqrt(2 delta / x^T (F + damping I) x): what step 4 computes already (tb_trpo_fvp adds the damping term).
  5'. theta_k = theta + beta 0.8^k x, k = 0 .. 9. The first k with finite entries, KL_k < delta and L_k > L_0 is taken, BOTH tests strict;
      L_0 is the surrogate at theta. It comes out of the search launch itself: a zero step stands in front of the candidates (K + 1
      <= 64 entries), whose KL is exactly 0.0 by the kernel's construction. select_candidate_sb3 chooses, on the device; a rejected
      step leaves theta bit-identical.
  6'. The critic: n_epochs = 10 (n_critic_updates) of Adam at learning_rate 1e-3 on the plain MSE (vf_coef = 1.0), gae_lambda 0.95,
      gamma 0.99, advantages normalised over the rollout, NO gradient-norm clip: max_grad_norm = inf, with which tb_ppo_apply's clip
      factor is exactly 1.0f and the gradient keeps its bits (tests/test_gpu_mlp64_learner.py).
Left to the script: num_envs, n_steps and the critic's minibatch size. sb3_contrib's 2048 steps of ONE env and its 128-row minibatches
are sized for one env, not for 4096 of them.
Deviations from sb3_contrib's TRPO.train, all of them:
  * CG's early exit at a residual below cg_tolerance is the device-side freeze above: the iterations run on, nothing moves.
  * The ratio's old log-probability is the rollout's own (as in the PPO learner), not a second forward pass of the old policy.
  * log_std is inside the natural gradient with its exact Fisher block 2 I (sb3_contrib differentiates the KL through it as well).
  * The critic's minibatches are the script's (above); sb3_contrib's early stop of the critic does not exist, there is none to port.

form="agent_returns": agent.py's own estimator and update, with nothing behind the trust-region step (AGENT_PY_DEFAULTS).
  0''. The collect is unchanged: PPOTrainer's fused rollout. The value tower still runs inside the rollout kernel and its output is
       ignored -- a cost this form pays for sharing the rollout kernels.
  1''. tb_trpo_returns replaces tb_ppo_gae: the discounted return-to-go (discount = 0.98, agent.py:17,264-268) of the episodes that ENDED
       inside this rollout -- an episode that began in an earlier rollout included --, float64 sums rounded to float32 once as
       agent.py's Python floats are (agent.py:200), with the flat indices of those finished rows, compacted on the device, and their
       count. The raw returns are the `adv` of tb_ppo_grad and tb_trpo_search, the index list their rows, the count their batch: both
       kernels normalise over exactly the rows they are given (mean, unbiased std), which is agent.py:210.
  2''. The CG rows are the first max(1, int(0.1 count)) entries of idx[randperm(count)] (agent.py:218-220).
  3''. log_std_step="raw" (agent.py:116-120,136,155-162): CG and the Fisher-vector products see the network's slots only (b and every
       p are 0 on log_std, where tb_trpo_fvp then gives 0); beta comes from that x; in the search direction the log_std slots hold g's:
       log_std_k = log_std + step_k g_logstd, the network's scalar step.
  4''. step_rows="all" (agent.py:110-111): the one product behind beta runs over all finished rows.
  5''. No critic: no value minibatch runs, n_epochs is ignored; the value slots of the parameters, the gradient and both Adam moments
       are not written, the optimiser's state is not touched. The report has value_loss = NaN.
  6''. log_std starts at log_std_init = exp(-1) (agent.py:39-42).
The launch arguments need the count on the host, so this form reads the device TWICE per update -- the count, then the statistics --
where the other forms read once. With fewer than two finished rows the policy step is skipped: theta stays bit-identical, the report
carries accepted_k = -1. The report also holds finished_rows and finished_share = finished_rows / rows.
Deviations of form="agent_returns" from agent.py, all of them:
  * The denominator of the normalisation is std + 1e-8 (the kernels'), agent.py:210 divides by std.
  * The unfinished tail of each env is dropped; agent.py:228-230 keeps it for the next batch, with its then stale log-probabilities.
  * max_episode_length (agent.py:261-262) does not exist: the envs end their episodes themselves.
  * The policy is the env's default network (and collects through it); agent.py takes any nn.Sequential.
  * CG's early exit is the device-side freeze; the ratio's old log-probability is the rollout's own; the CG rows come from a
    device-side torch.randperm -- as in form="agent", above.
"""
import math

from .learner import TB_PPO_REDUCE, TB_PPO_STEP, FusedLearner, flatten_parameters, parameter_offsets
from .ppo import SB3_SWING_DEFAULTS, SWING_DEFAULTS, TENNIS_DEFAULTS, PPOTrainer
from .params import ENV_SWING
from .stepper import ENV_IDS, StepperError, _check

TB_PPO_VALUE_ONLY = 4
TRPO_DEFAULTS = dict(kl_delta=0.01, cg_iterations=10, cg_damping=0.001, cg_tolerance=1e-10, cg_state_percent=0.1,   # agent.py:17-18
                     search_candidates=10, search_decay=1.5)                                                      # agent.py:112-113
# [3P-recalled] sb3_contrib 1.8.0, TRPO.__init__'s defaults (the package is not installed here: a host that has it corrects them in
# this one place). search_decay 1.25 = 1 / line_search_shrinking_factor 0.8; cg_state_percent 1.0 = sub_sampling_factor 1;
# search_candidates = line_search_max_iter; cg_iterations = cg_max_steps; kl_delta = target_kl; n_epochs = n_critic_updates.
SB3_TRPO_DEFAULTS = dict(kl_delta=0.01, cg_iterations=15, cg_damping=0.1, cg_tolerance=1e-10, cg_state_percent=1.0, search_candidates=10, search_decay=1.25,
                         n_epochs=10, learning_rate=1e-3, vf_coef=1.0, gae_lambda=0.95, gamma=0.99, max_grad_norm=float("inf"))
# form="agent_returns": TRPOAgent.__init__'s and line_search's constants, as above, and what agent.py does where form="agent" does not
AGENT_PY_DEFAULTS = dict(TRPO_DEFAULTS,
                         discount=0.98,                # agent.py:17 (used at agent.py:264-268)
                         log_std_step="raw",           # agent.py:120,136: logstd + step_size * logstd.grad
                         step_rows="all",              # agent.py:110-111: fisher_vector_direct(gradients, states) over every state
                         log_std_init=math.exp(-1))    # agent.py:39-42: ones / ones.exp()
FORMS = ("agent", "sb3", "agent_returns")
LOG_STD_STEPS, STEP_ROWS = ("natural", "raw"), ("cg", "all")
_PRESETS = {"agent": TRPO_DEFAULTS, "sb3": SB3_TRPO_DEFAULTS, "agent_returns": AGENT_PY_DEFAULTS}
_FORM_ERROR = "form must be 'agent', 'sb3' or 'agent_returns', not %r"


def form_keywords(form, kw):
    """TRPOTrainer's keywords with the form's preset under them: form="sb3" and form="agent_returns" preset every hyper-parameter their
    dict names, and an explicit keyword wins; form="agent" presets nothing here (TRPO_DEFAULTS fills what is left, as always)"""
    return dict({"sb3": SB3_TRPO_DEFAULTS, "agent_returns": AGENT_PY_DEFAULTS}.get(form, {}), **kw)


def raw_log_std_direction(torch, xf, g, log_std_mask):
    """log_std_step="raw": the search direction whose network slots are xf's (the natural-gradient solve, 0 on log_std) and whose
    log_std slots are g's, so that theta + step * direction moves log_std by step * g_logstd (agent.py:120,136)"""
    return torch.where(log_std_mask, g, xf).contiguous()


def skip_update(finished_rows):
    """form="agent_returns": no policy step on fewer than two finished rows (agent.py:194-196 returns on none; one row has no
    unbiased std, and tb_ppo_grad refuses it)"""
    return int(finished_rows) < 2


def select_candidate(torch, table, delta):
    """table [K, 2] = (L_k, KL_k), a tensor: the first k that is finite with KL_k <= delta and L_k >= 0 (agent.py:132), or -1;
    a 0-d int64 tensor on the table's device"""
    K = table.shape[0]
    L, KL = table[:, 0], table[:, 1]
    ok = torch.isfinite(L) & torch.isfinite(KL) & (KL <= delta) & (L >= 0)
    first = torch.where(ok, torch.arange(K, device=table.device), torch.full((K,), K, device=table.device)).min()
    return torch.where(first < K, first, torch.full_like(first, -1))


def select_candidate_sb3(torch, table, delta):
    """sb3_contrib's rule. table [K + 1, 2] = (L, KL), row 0 the zero step (L_0, 0.0), rows 1 .. K the candidates: the first candidate
    k (0-based among the candidates) that is finite with KL_k < delta and L_k > L_0 -- both strict -- or -1; a 0-d int64 tensor on
    the table's device"""
    K = table.shape[0] - 1
    L0, L, KL = table[0, 0], table[1:, 0], table[1:, 1]
    ok = torch.isfinite(L) & torch.isfinite(KL) & (KL < delta) & (L > L0)
    first = torch.where(ok, torch.arange(K, device=table.device), torch.full((K,), K, device=table.device)).min()
    return torch.where(first < K, first, torch.full_like(first, -1))


class FusedTRPO(FusedLearner):
    """GAE (inherited), the trust-region policy step and the critic's epochs on the device for one policy / optimiser pair"""

    def __init__(self, kind, policy, opt, hp, device, form="agent"):
        if hasattr(policy, "features_extractor"):
            raise ValueError("FusedTRPO needs the env's default net_arch: its kernels are not instantiated for the tuned network")
        if form not in FORMS:
            raise ValueError(_FORM_ERROR % (form,))
        self.form = form
        for k, v in _PRESETS[form].items():  # filled in place: hp stays the caller's dict, as with FusedLearner, so a later change of
            if k in AGENT_PY_DEFAULTS:       # trainer.hp reaches the learner
                hp.setdefault(k, v)
        hp.setdefault("log_std_step", "natural")
        hp.setdefault("step_rows", "cg")
        if hp["log_std_step"] not in LOG_STD_STEPS or hp["step_rows"] not in STEP_ROWS:
            raise ValueError("FusedTRPO: log_std_step 'natural' or 'raw' and step_rows 'cg' or 'all' expected, not %r and %r" % (hp["log_std_step"], hp["step_rows"]))
        super().__init__(kind, policy, opt, hp, device)
        t = self.torch
        self._zero = 1 if form == "sb3" else 0    # entries in front of the candidates: sb3's zero step, whose L is L_0
        if not 1 <= int(self.hp["search_candidates"]) <= 64 - self._zero or int(self.hp["cg_iterations"]) < 1 or not 0.0 < float(self.hp["cg_state_percent"]) <= 1.0:
            raise ValueError("FusedTRPO: search_candidates 1 .. 64 (form='sb3': 63, the zero step being one entry), cg_iterations >= 1 and 0 < cg_state_percent <= 1 expected")
        self.mask = t.zeros(self.n_params, dtype=t.float32, device=self.device)   # 1 on theta's slots
        for name, (off, n) in parameter_offsets(policy).items():
            if name == "log_std" or name.startswith("policy_net.") or name.startswith("action_net."):
                self.mask[off:off + n] = 1.0
        z = lambda n, dt=t.float32: t.zeros(n, dtype=dt, device=self.device)  # noqa: E731
        self._g, self._gstats, self._fv, self._fx = z(self.n_params), z(3), z(self.n_params), z(self.n_params)
        K = int(self.hp["search_candidates"])
        self.table = z((K + self._zero, 2), t.float64)
        self._decay = t.tensor([float(self.hp["search_decay"]) ** -k for k in range(K)], dtype=t.float64, device=self.device)
        self.report = z(5, t.float64)
        self._fvp_ws = self._search_ws = self._rows = self._returns_ws = None
        self._log_std = t.zeros(self.n_params, dtype=t.bool, device=self.device)   # log_std's slots; net_mask: theta without them
        off, n = parameter_offsets(policy)["log_std"]
        self._log_std[off:off + n] = True
        self.net_mask = self.mask * (~self._log_std).float()

    # ----------------------------------------------------------------------------------------------------------- the kernels
    def fvp(self, obs, idx_ptr, m, vec, out, damping=None):
        """out = F vec + damping vec over the rows idx[0 .. m) (a device pointer to int64) of obs; returns out"""
        obs, vec = self._float(obs, "obs"), self._float(vec, "vec")
        if out.dtype != self.torch.float32 or out.device != self.flat.device or not out.is_contiguous() or out.numel() != self.n_params or vec.numel() != self.n_params:
            raise ValueError("fvp: vec and out must be contiguous float32 vectors of %d floats on %s" % (self.n_params, self.flat.device))
        self._fvp_ws = ws = self._grow(self._fvp_ws, self.lib.tb_trpo_fvp_workspace_bytes_net(self.kind, self.net, int(m)), "tb_trpo_fvp_workspace_bytes")
        _check(self.lib, self.lib.tb_trpo_fvp_net(self.kind, self.net, self._dev(), self._stream(), obs.data_ptr(), int(obs.shape[0]), idx_ptr, int(m), self.flat.data_ptr(),
                                              vec.data_ptr(), self.n_params, float(self.hp["cg_damping"] if damping is None else damping), out.data_ptr(),
                                              ws.data_ptr(), ws.numel() * 8), "tb_trpo_fvp")
        return out

    def search(self, arrays, n_rows, idx_ptr, batch, direction, steps, out=None):
        """(L_k, KL_k) of theta + steps[k] * direction over the rows idx[0 .. batch): a float64 [K, 2] tensor"""
        t = self.torch
        obs, act, old_logp, adv = arrays[:4]
        direction, steps = self._float(direction, "direction"), self._float(steps, "steps")
        K = int(steps.numel())
        if direction.numel() != self.n_params:
            raise ValueError("search: the direction must hold %d floats" % self.n_params)
        out = out if out is not None else t.zeros((K, 2), dtype=t.float64, device=self.device)
        self._search_ws = ws = self._grow(self._search_ws, self.lib.tb_trpo_search_workspace_bytes_net(self.kind, self.net, int(batch), K), "tb_trpo_search_workspace_bytes")
        _check(self.lib, self.lib.tb_trpo_search_net(self.kind, self.net, self._dev(), self._stream(), obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), int(n_rows),
                                                 idx_ptr, int(batch), self.flat.data_ptr(), direction.data_ptr(), self.n_params, steps.data_ptr(), K, out.data_ptr(),
                                                 ws.data_ptr(), ws.numel() * 8), "tb_trpo_search")
        return out

    def surrogate_gradient(self, arrays, n_rows, idx_ptr, batch):
        """g = grad_theta mean(ratio A_hat) over the rows idx[0 .. batch), 0 on the value slots: minus what tb_ppo_grad leaves
        when its clip never binds. self.grad is not touched."""
        L, dev, s = self.lib, self._dev(), self._stream()
        obs, act, old_logp, adv, returns = arrays
        ws = self.workspace(batch)
        wb = ws.numel() * 8
        _check(L, L.tb_ppo_grad_net(self.kind, self.net, dev, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), returns.data_ptr(), n_rows, idx_ptr, batch,
                                self.flat.data_ptr(), self.n_params, float("inf"), 0.0, ws.data_ptr(), wb), "tb_ppo_grad")
        _check(L, L.tb_ppo_apply_net(self.kind, self.net, dev, s, TB_PPO_REDUCE, ws.data_ptr(), wb, batch, self.flat.data_ptr(), self._g.data_ptr(), None, None, self.n_params,
                                 self._gstats.data_ptr(), 0.0, 1.0, 1, 0.0, 0.9, 0.999, 1e-5, 1), "tb_ppo_apply")
        return -self._g * self.mask

    def conjugate_gradient(self, b, obs, idx_ptr, m):
        """x ~ (F + damping)^-1 b, agent.py:169-191; float64 [P]. Frozen (not left) once rdotr < cg_tolerance."""
        t = self.torch
        p, r = b.clone(), b.double()
        x = t.zeros_like(r)
        rdotr = r.dot(r)
        live = t.ones((), dtype=t.bool, device=self.device)
        tol = float(self.hp["cg_tolerance"])
        for _ in range(int(self.hp["cg_iterations"])):
            pd = p.double()
            f = self.fvp(obs, idx_ptr, m, p, self._fv).double()
            alpha = rdotr / pd.dot(f)
            x = t.where(live, x + alpha * pd, x)
            r_new = r - alpha * f
            new_rdotr = r_new.dot(r_new)
            p = t.where(live, (r_new + (new_rdotr / rdotr) * pd).float(), p)
            r = t.where(live, r_new, r)
            rdotr = t.where(live, new_rdotr, rdotr)
            live = live & (rdotr >= tol)
        return x

    def policy_step(self, arrays, n_rows, all_ptr, cg_ptr, m, batch=None):
        """steps 1-5 of the module docstring over the rows all[0 .. batch) (batch: n_rows unless given), the Fisher-vector products on
        cg[0 .. m); theta moves in place (or not at all). Returns (accepted k or -1, L, KL of the accepted candidate -- of k = 0 when
        none is) as 0-d device tensors. No host synchronisation."""
        t, hp = self.torch, self.hp
        batch = int(n_rows if batch is None else batch)
        raw = hp["log_std_step"] == "raw"
        g = self.surrogate_gradient(arrays, n_rows, all_ptr, batch)
        mask = self.net_mask if raw else self.mask    # raw: CG sees the network's slots alone, 0 on log_std stays 0 through tb_trpo_fvp
        x = self.conjugate_gradient(g * mask if raw else g, arrays[0], cg_ptr, m)
        xf = (x.float() * mask).contiguous()
        if hp["step_rows"] == "all":                  # agent.py:110-111: x^T F x over every row of the step
            xFx = xf.double().dot(self.fvp(arrays[0], all_ptr, batch, xf, self._fx).double())
        else:
            xFx = xf.double().dot(self.fvp(arrays[0], cg_ptr, m, xf, self._fx).double())
        beta = t.sqrt(2.0 * float(hp["kl_delta"]) / xFx)
        steps = (beta * self._decay).float()
        if self._zero:                                # form="sb3": the zero step in front, table[0] = (L_0, 0.0)
            steps = t.cat([t.zeros(1, dtype=t.float32, device=self.device), steps])
        if raw:
            xf = raw_log_std_direction(t, xf, g, self._log_std)
        self.search(arrays, n_rows, all_ptr, batch, xf, steps, out=self.table)
        k = (select_candidate_sb3 if self._zero else select_candidate)(t, self.table, float(hp["kl_delta"]))
        accepted = k >= 0
        kk = (k.clamp(min=0) + self._zero).view(1)    # (gather / index_select: indexing with a 0-d tensor would read it on the host)
        moved = self.flat + steps.gather(0, kk) * xf  # the product and the sum rounded separately: what the search kernel evaluated
        self.flat.copy_(t.where(accepted, moved, self.flat))
        self.gradient, self.direction, self.steps = g, xf, steps   # this step's, for whoever checks it
        row = self.table.index_select(0, kk)[0]
        return k, row[0], row[1]

    # ----------------------------------------------------------------------------------------- form="agent_returns": the estimator
    def returns_to_go(self, rewards, dones):
        """tb_trpo_returns on a rollout's rewards / dones [T, n] (strided over steps as `advantages` takes them): (returns float32
        [T, n] -- 0 on unfinished rows --, idx int64 [T n] whose first `count` entries are the finished rows' flat indices in
        ascending order, count int64 [1]); all on the device, nothing is read"""
        t = self.torch
        T, n = rewards.shape
        if dones.dtype == t.bool:
            dones = dones.view(t.uint8)
        if rewards.dtype != t.float32 or dones.dtype != t.uint8 or tuple(dones.shape) != (T, n) or rewards.device != self.flat.device or dones.device != self.flat.device:
            raise ValueError("returns_to_go: rewards float32 [T, n] and dones uint8 [T, n] on %s expected" % self.flat.device)
        if n > 1 and rewards.stride(1) != 1 or T > 1 and rewards.stride(0) < n:
            rewards = rewards.contiguous()
        if n > 1 and dones.stride(1) != 1 or T > 1 and dones.stride(0) < n:
            dones = dones.contiguous()
        r_stride = 4 * rewards.stride(0) if T > 1 else 0
        d_stride = dones.stride(0) if T > 1 else 0
        returns = t.empty((T, n), dtype=t.float32, device=self.device)
        idx, count = t.empty(T * n, dtype=t.int64, device=self.device), t.zeros(1, dtype=t.int64, device=self.device)
        self._returns_ws = ws = self._grow(self._returns_ws, self.lib.tb_trpo_returns_workspace_bytes(int(T), int(n)), "tb_trpo_returns_workspace_bytes")
        _check(self.lib, self.lib.tb_trpo_returns(self.kind, self._dev(), self._stream(), int(T), int(n), rewards.data_ptr(), r_stride, dones.data_ptr(), d_stride,
                                                  float(self.hp.get("discount", AGENT_PY_DEFAULTS["discount"])), returns.data_ptr(), idx.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 8), "tb_trpo_returns")
        return returns, idx, count

    def update_finished(self, obs, act, old_logp, returns, idx, count):
        """form="agent_returns": one trust-region step on the finished rows idx[0 .. count) of the flat rollout [n, ...], weighted by
        the raw `returns` (the kernels normalise over those rows); no critic. Draws one torch.randperm(count). Reads the device
        twice: the count, a launch argument, and the statistics at the end. count < 2: no step, theta bit for bit as it was."""
        t = self.torch
        n = int(returns.shape[0])
        arrays = tuple(self._float(x, name) for x, name in ((obs, "obs"), (act, "act"), (old_logp, "old_logp"), (returns, "returns")))
        arrays = arrays + (arrays[3],)   # tb_ppo_grad's `returns`: the value loss's target, weighted by vf_coef = 0.0 there
        if arrays[0].numel() * self.lib.tb_act_dim(self.kind) != arrays[1].numel() * self.lib.tb_obs_dim(self.kind) or arrays[0].shape[0] != n \
                or any(int(x.numel()) != n for x in arrays[2:]) or idx.dtype != t.int64 or idx.numel() < n or not idx.is_contiguous() or count.dtype != t.int64:
            raise ValueError("update_finished: obs [n, O], act [n, A], old_logp / returns [n], idx int64 [n] and count int64 [1] expected")
        flatten_parameters(self.policy)
        if self.policy._flat_params is not self.flat:
            self.flat = self.policy._flat_params
        finished = int(count.item())     # the first device-to-host read: the kernels' batch
        if not 0 <= finished <= n:
            raise StepperError("update_finished: count = %d outside 0 .. %d" % (finished, n))
        nan = float("nan")
        out = {"accepted_k": -1, "surrogate": nan, "kl": nan, "policy_loss": nan, "value_loss": nan, "entropy": nan,
               "finished_rows": finished, "finished_share": finished / n}
        if skip_update(finished):
            return out
        m = max(1, int(float(self.hp["cg_state_percent"]) * finished))
        cg_rows = idx[:finished].index_select(0, t.randperm(finished, device=self.device))
        k, L, KL = self.policy_step(arrays, n, idx.data_ptr(), cg_rows.data_ptr(), m, batch=finished)
        off, A = parameter_offsets(self.policy)["log_std"]
        self.report[0], self.report[1], self.report[2] = k.double(), L, KL
        self.report[3] = nan
        self.report[4] = (0.5 + 0.5 * math.log(2.0 * math.pi)) * A + self.flat[off:off + A].double().sum()   # the moved policy's entropy
        k, L, KL, vl, ent = self.report.tolist()  # the second device-to-host read
        out.update(accepted_k=int(k), surrogate=L, kl=KL, policy_loss=-L, entropy=ent)
        return out

    def value_minibatch(self, arrays, n_rows, idx_ptr, batch, step):
        """one Adam step of the critic alone on rows idx[0 .. batch)"""
        L, hp, dev, s = self.lib, self.hp, self._dev(), self._stream()
        obs, act, old_logp, adv, returns = arrays
        ws = self.workspace(batch)
        wb = ws.numel() * 8
        _check(L, L.tb_ppo_grad_net(self.kind, self.net, dev, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), returns.data_ptr(), n_rows, idx_ptr, batch,
                                self.flat.data_ptr(), self.n_params, float(hp["clip_range"]), float(hp["vf_coef"]), ws.data_ptr(), wb), "tb_ppo_grad")
        g = self.opt.param_groups[0]
        _check(L, L.tb_ppo_apply_net(self.kind, self.net, dev, s, TB_PPO_REDUCE | TB_PPO_STEP | TB_PPO_VALUE_ONLY, ws.data_ptr(), wb, batch, self.flat.data_ptr(), self.grad.data_ptr(),
                                 self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.n_params, self.stats.data_ptr(), float(hp["ent_coef"]),
                                 float(hp["max_grad_norm"]), 1, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), int(step)), "tb_ppo_apply")

    # ---------------------------------------------------------------------------------------------------------------- update
    def update(self, obs, act, old_logp, adv, returns, n_epochs, batch_size, world=1):
        """one trust-region step of the policy on the flat rollout [n, ...], then n_epochs of the critic in minibatches of
        batch_size rows. Draws one torch.randperm(n) for the CG rows and one per critic epoch; reads the device once, at the end."""
        t = self.torch
        if int(world) != 1:
            raise StepperError("FusedTRPO: one rank only (multi-rank TRPO is not provided)")
        if self.form == "agent_returns":
            raise StepperError("FusedTRPO: form='agent_returns' has no critic and no advantages; its update is update_finished (returns_to_go's outputs)")
        n = int(adv.shape[0])
        arrays = tuple(self._float(x, name) for x, name in ((obs, "obs"), (act, "act"), (old_logp, "old_logp"), (adv, "adv"), (returns, "returns")))
        if arrays[0].numel() * self.lib.tb_act_dim(self.kind) != arrays[1].numel() * self.lib.tb_obs_dim(self.kind) or arrays[0].shape[0] != n \
                or any(int(x.numel()) != n for x in arrays[2:]):
            raise ValueError("update: obs [n, O], act [n, A], old_logp / adv / returns [n] expected")
        flatten_parameters(self.policy)
        if self.policy._flat_params is not self.flat:
            self.flat = self.policy._flat_params
        step = self._adopt_optimizer_state()
        if self._rows is None or self._rows.numel() != n:
            self._rows = t.arange(n, device=self.device)
        m = max(1, int(float(self.hp["cg_state_percent"]) * n))
        cg_rows = t.randperm(n, device=self.device)
        k, L, KL = self.policy_step(arrays, n, self._rows.data_ptr(), cg_rows.data_ptr(), m)
        for _ in range(int(n_epochs)):
            perm = t.randperm(n, device=self.device)
            for s in range(0, n, int(batch_size)):
                if n - s < 2:
                    break  # (a tail of one row has no unbiased std; tb_ppo_grad refuses it)
                step += 1
                self.value_minibatch(arrays, n, perm.data_ptr() + 8 * s, min(int(batch_size), n - s), step)
        for p, (gv, mv, vv) in zip(self.params, self._views):
            st = self.opt.state[p]
            st["step"] = t.tensor(float(step), dtype=st["step"].dtype, device=st["step"].device)
            p.grad = gv
        self.report[0], self.report[1], self.report[2] = k.double(), L, KL
        self.report[3:5] = self.stats[1:3].double()
        k, L, KL, vl, ent = self.report.tolist()  # the one device-to-host read
        return {"accepted_k": int(k), "surrogate": L, "kl": KL, "policy_loss": -L, "value_loss": vl, "entropy": ent}


class TRPOTrainer(PPOTrainer):
    """TRPO over a BatchedEnv: PPOTrainer's collect, GAE and critic; the policy moves by FusedTRPO's trust-region step.
    hp: kl_delta, cg_iterations, cg_damping, cg_state_percent (TRPO_DEFAULTS) beside PPOTrainer's.
    form="agent": the reference's agent.py; form="sb3": sb3_contrib's TRPO with SB3_TRPO_DEFAULTS as the preset of every hyper-parameter
    it names (an explicit keyword wins). policy="mlp64": SB3's [64, 64] on SwingRacket-v0 -- with form="sb3" the reference's
    `train_swing.py -s trpo`. form="agent_returns": agent.py without a critic -- discounted returns of finished episodes
    (tb_trpo_returns), AGENT_PY_DEFAULTS as the preset, an explicit keyword wins; the rollout kernel's value tower runs and is
    ignored, and an update reads the device twice (the module docstring). log_std_step ("natural" | "raw"), step_rows ("cg" | "all")
    and log_std_init are hyper-parameters of every form; "agent" and "sb3" default to "natural", "cg" and the module's own 0."""

    def __init__(self, env_id="SwingRacket-v0", num_envs=4096, n_steps=104, device=None, seed=0, batch_size=None, form="agent", **kw):
        import torch
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("TRPOTrainer runs on one rank (world size %d): multi-rank TRPO is not provided" % dist.get_world_size())
        if form not in FORMS:
            raise ValueError(_FORM_ERROR % (form,))
        mlp64 = kw.get("policy", "default") == "mlp64"   # (on another env than SwingRacket-v0: PPOTrainer's refusal, by name)
        default_arch = tuple((SB3_SWING_DEFAULTS if mlp64 else SWING_DEFAULTS if ENV_IDS[env_id] == ENV_SWING else TENNIS_DEFAULTS)["net_arch"])
        if tuple(kw.get("net_arch", default_arch)) != default_arch or not kw.get("fused", True) or kw.get("policy", "default") not in ("default", "mlp64"):
            raise ValueError("TRPOTrainer needs the env's default net_arch %s (or policy='mlp64' on SwingRacket-v0) and the fused rollout: its kernels are "
                             "instantiated for those architectures" % (default_arch,))
        if kw.pop("learner", "fused") != "fused":
            raise ValueError("TRPOTrainer has no torch learner")
        kw = form_keywords(form, kw)
        for key, allowed in (("log_std_step", LOG_STD_STEPS), ("step_rows", STEP_ROWS)):
            if kw.get(key, allowed[0]) not in allowed:
                raise ValueError("TRPOTrainer: %s must be one of %s, not %r" % (key, allowed, kw[key]))
        super().__init__(env_id, num_envs, n_steps, device, seed, batch_size, learner="torch", **kw)
        self.form = form
        self.hp = dict(TRPO_DEFAULTS, **self.hp)
        if self.hp.get("log_std_init") is not None:   # (build_actor_critic takes none: set on the module, before the learner flattens it)
            with torch.no_grad():
                self.policy.log_std.fill_(float(self.hp["log_std_init"]))
        self._learner = FusedTRPO(ENV_IDS[env_id], self.policy, self.opt, self.hp, self.device, form=form)
        self._finished = None

    def advantages(self, last_value):
        """form="agent_returns": (returns, returns) of tb_trpo_returns -- there are no advantages and last_value is not used --, the
        finished rows' index list kept for `update`; the other forms: PPOTrainer's GAE"""
        if self.form != "agent_returns":
            return super().advantages(last_value)
        returns, idx, count = self._learner.returns_to_go(self.buf.rewards, self.buf.dones)
        self._finished = (returns, idx, count)
        return returns, returns

    def update(self, adv, returns):
        if self.form != "agent_returns":
            return super().update(adv, returns)
        if self._finished is None or returns is not self._finished[0]:
            raise StepperError("TRPOTrainer(form='agent_returns').update takes what ITS advantages() returned: the finished rows' index list belongs to those returns")
        n = self.n_steps * self.num_envs
        _, idx, count = self._finished
        self._last_update = self._learner.update_finished(self.obs_seq.reshape(n, -1), self._raw_actions.reshape(n, -1), self.logps.reshape(n), returns.reshape(n), idx, count)
        return dict(self._last_update)

    def learn(self, total_timesteps, log=print, **kw):
        """PPOTrainer.learn; form="agent_returns" adds the share of finished rows and the accepted candidate to the progress line"""
        if self.form == "agent_returns" and log:
            inner = log
            log = lambda line: inner("%s  finished share %.3f  accepted k %d" % (line, self._last_update["finished_share"], self._last_update["accepted_k"]))  # noqa: E731
        return super().learn(total_timesteps, log=log, **kw)
