"""The PPO learner as HIP kernels (csrc/tb_learner.hpp; C ABI tb_ppo_gae / tb_ppo_grad / tb_ppo_apply in include/tb_stepper.h).

`PPOTrainer(..., learner="fused")` hands `advantages` and `update` to a `FusedLearner` -- for the env's default network or, with
policy="tuned", Tennisbot's tuned one (the `_net` entry points; the module tells which). The kernels work on ONE flat fp32 parameter
vector, so `flatten_parameters` first re-points every parameter of the torch module at a view of one buffer, in
`named_parameters()` order: the module, its state_dict, `pack_policy` and a torch optimiser see the same tensors as before.
The gradient and both Adam moments live in flat buffers of the same order; `p.grad` and `opt.state[p]` hold views of them,
so checkpoints, a switch of learners mid-run and readers of the optimiser's state keep working.

Per minibatch: tb_ppo_grad (advantage statistics, then the gradient kernel: rows gathered by the workgroups themselves),
tb_ppo_apply (fixed-order reduction, norm clip, Adam) -- four launches, no host synchronisation; with several ranks ONE
all_reduce of the flat gradient between the reduction and the clip. There is no torch fallback: a refused call raises.
"""
from .stepper import StepperError, _check, load_library

TB_PPO_REDUCE, TB_PPO_STEP = 1, 2


def parameter_offsets(policy):
    """name -> (offset, numel) in the flat vector: named_parameters() order, each tensor row-major"""
    out, off = {}, 0
    for name, p in policy.named_parameters():
        out[name] = (off, p.numel())
        off += p.numel()
    return out


def flatten_parameters(policy):
    """Re-point every parameter's .data at a view of one contiguous float32 buffer (returned; also kept as
    policy._flat_params). Values, names, forward, load_state_dict and pack_policy are unaffected. Pure torch."""
    import torch
    params = [p for _, p in policy.named_parameters()]
    flat = getattr(policy, "_flat_params", None)
    total = sum(p.numel() for p in params)
    if flat is not None and flat.numel() == total and flat.device == params[0].device:
        off, aliased = 0, True
        for p in params:
            aliased = aliased and p.data_ptr() == flat.data_ptr() + 4 * off and p.is_contiguous()
            off += p.numel()
        if aliased:
            return flat
    if any(p.dtype != torch.float32 for p in params):
        raise ValueError("flatten_parameters: float32 parameters only")
    flat = torch.empty(total, dtype=torch.float32, device=params[0].device)
    off = 0
    with torch.no_grad():
        for p in params:
            view = flat[off:off + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            off += p.numel()
    policy._flat_params = flat
    return flat


# What every learner object (FusedLearner and FusedTRPO, PopulationPPO) needs around a library call; each takes them as methods: they
# read self.torch, self.device and self.lib.
def current_stream(self):
    return self.torch.cuda.current_stream(self.device).cuda_stream


def device_index(self):
    return self.device.index if self.device.index is not None else self.torch.cuda.current_device()


def grown_workspace(self, ws, need, what):
    """`ws` if it holds `need` bytes (the answer of the C query `what`: a refusal raises), else a new zeroed float64 one that does"""
    if need < 0:
        _check(self.lib, int(need), what)
    if ws is None or ws.numel() * 8 < need:
        ws = self.torch.zeros((need + 7) // 8, dtype=self.torch.float64, device=self.device)
    return ws


def gae(self, rewards, dones, values, last_value):
    """(adv, returns) float32 [T, n] of tb_ppo_gae with self.hp's gamma and gae_lambda. rewards float32 / dones uint8 [T, n] with
    contiguous rows, which may be strided over steps (a packed rollout buffer's views); values [T, n] and last_value [n] contiguous."""
    t = self.torch
    T, n = values.shape
    r_stride = 4 * rewards.stride(0) if T > 1 and rewards.stride(0) >= n else 0
    d_stride = dones.stride(0) if T > 1 and dones.stride(0) >= n else 0
    if T > 1 and (rewards.stride(0) < n or dones.stride(0) < n):
        rewards, dones, r_stride, d_stride = rewards.contiguous(), dones.contiguous(), 0, 0
    adv, returns = t.empty((T, n), dtype=t.float32, device=self.device), t.empty((T, n), dtype=t.float32, device=self.device)
    _check(self.lib, self.lib.tb_ppo_gae(self.kind, self._dev(), self._stream(), T, n, rewards.data_ptr(), r_stride, dones.data_ptr(), d_stride,
                                         values.data_ptr(), last_value.data_ptr(), float(self.hp["gamma"]), float(self.hp["gae_lambda"]),
                                         adv.data_ptr(), returns.data_ptr()), "tb_ppo_gae")
    return adv, returns


class FusedLearner:
    """GAE and the PPO update on the device for one policy / optimiser pair. Needs no env."""
    _stream, _dev, _grow = current_stream, device_index, grown_workspace

    def __init__(self, kind, policy, opt, hp, device):
        import torch
        from .ppo import policy_net_of
        self.torch, self.kind, self.policy, self.opt, self.hp = torch, int(kind), policy, opt, hp
        # NET_TUNED for build_tuned_actor_critic's module: its own gradient kernel, shared-trunk partials; NET_MLP64 for SwingRacket's [64, 64]
        self.net = policy_net_of(policy)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise StepperError("FusedLearner needs a GPU (there is no CPU fallback)")
        self.lib = load_library()
        self.n_params = self.lib.tb_ppo_param_floats_net(self.kind, self.net)
        if self.n_params < 0:
            _check(self.lib, self.n_params, "tb_ppo_param_floats_net")
        self.params = [p for _, p in policy.named_parameters()]
        if self.n_params != sum(p.numel() for p in self.params):
            raise StepperError("the policy has %d parameters, the learner kernels of this env kind take %d (another net_arch?)"
                               % (sum(p.numel() for p in self.params), self.n_params))
        g = opt.param_groups
        if len(g) != 1 or [id(p) for p in g[0]["params"]] != [id(p) for p in self.params]:
            raise StepperError("FusedLearner: the optimiser must hold the policy's parameters in named_parameters() order, in one group")
        if g[0].get("amsgrad") or g[0].get("weight_decay") or g[0].get("maximize"):
            raise StepperError("FusedLearner: plain Adam only (no amsgrad, weight decay or maximize)")
        self.flat = flatten_parameters(policy)
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)  # noqa: E731
        self.grad, self.exp_avg, self.exp_avg_sq, self.stats = z(self.n_params), z(self.n_params), z(self.n_params), z(3)
        self._views = []
        off = 0
        for p in self.params:
            n = p.numel()
            self._views.append(tuple(b[off:off + n].view(p.shape) for b in (self.grad, self.exp_avg, self.exp_avg_sq)))
            off += n
        self._ws = None

    def _float(self, x, name):
        t = self.torch
        if x.dtype != t.float32 or x.device != self.flat.device:
            raise ValueError("%s: float32 tensor on %s expected" % (name, self.flat.device))
        return x if x.is_contiguous() else x.contiguous()

    # ---------------------------------------------------------------------------------------------------------------- GAE
    def advantages(self, rewards, values, dones, last_value):
        """(adv, returns), both [T, n]. rewards / dones may be strided over steps (a packed rollout buffer's views)."""
        t = self.torch
        T, n = values.shape
        values, last_value = self._float(values, "values"), self._float(last_value, "last_value")
        if dones.dtype == t.bool:
            dones = dones.view(t.uint8)
        if rewards.dtype != t.float32 or dones.dtype != t.uint8 or tuple(rewards.shape) != (T, n) or tuple(dones.shape) != (T, n) or tuple(last_value.shape) != (n,):
            raise ValueError("advantages: rewards float32 [T, n], dones uint8 [T, n], last_value [n] expected")
        if n > 1 and rewards.stride(1) != 1:
            rewards = rewards.contiguous()
        if n > 1 and dones.stride(1) != 1:
            dones = dones.contiguous()
        return gae(self, rewards, dones, values, last_value)

    # ------------------------------------------------------------------------------------------------------------- update
    def _adopt_optimizer_state(self):
        """the moments as the optimiser holds them NOW (opt.load_state_dict replaces its tensors) into the flat buffers, and
        the flat buffers' views back into opt.state; returns the number of steps taken so far"""
        t = self.torch
        step = None
        for p, (gv, mv, vv) in zip(self.params, self._views):
            st = self.opt.state[p]
            if len(st) == 0:
                mv.zero_(); vv.zero_()
                st["step"] = t.tensor(0.0)
            else:
                if st["exp_avg"].data_ptr() != mv.data_ptr():
                    mv.copy_(st["exp_avg"])
                if st["exp_avg_sq"].data_ptr() != vv.data_ptr():
                    vv.copy_(st["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = mv, vv
            k = int(st["step"])
            if step is not None and k != step:
                raise StepperError("FusedLearner: the optimiser's parameters have taken different numbers of steps")
            step = k
        return step

    def workspace(self, batch):
        self._ws = self._grow(self._ws, self.lib.tb_ppo_workspace_bytes_net(self.kind, self.net, int(batch)), "tb_ppo_workspace_bytes_net")
        return self._ws

    def minibatch(self, arrays, n_rows, idx_ptr, batch, step, world=1):
        """one gradient step on rows idx[0 .. batch) (a device pointer to int64); `step`: the 1-based count of this Adam step"""
        L, hp, dev, s = self.lib, self.hp, self._dev(), self._stream()
        obs, act, old_logp, adv, returns = arrays
        ws = self.workspace(batch)
        wb = ws.numel() * 8
        _check(L, L.tb_ppo_grad_net(self.kind, self.net, dev, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), returns.data_ptr(), n_rows,
                                idx_ptr, batch, self.flat.data_ptr(), self.n_params, float(hp["clip_range"]), float(hp["vf_coef"]), ws.data_ptr(), wb), "tb_ppo_grad")
        g = self.opt.param_groups[0]
        tail = (self.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.n_params, self.stats.data_ptr(),
                float(hp["ent_coef"]), float(hp["max_grad_norm"]), int(world), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), int(step))
        if world > 1:  # the average first, the clip second: ONE collective on the flat gradient
            _check(L, L.tb_ppo_apply_net(self.kind, self.net, dev, s, TB_PPO_REDUCE, ws.data_ptr(), wb, batch, *tail), "tb_ppo_apply")
            self.torch.distributed.all_reduce(self.grad)
            _check(L, L.tb_ppo_apply_net(self.kind, self.net, dev, s, TB_PPO_STEP, ws.data_ptr(), wb, batch, *tail), "tb_ppo_apply")
        else:
            _check(L, L.tb_ppo_apply_net(self.kind, self.net, dev, s, TB_PPO_REDUCE | TB_PPO_STEP, ws.data_ptr(), wb, batch, *tail), "tb_ppo_apply")

    def update(self, obs, act, old_logp, adv, returns, n_epochs, batch_size, world=1):
        """n_epochs over the flat rollout [n, ...] in minibatches of batch_size rows (a ragged tail included). Draws exactly one
        torch.randperm(n) per epoch; reads the device once, at the end, for the statistics of the last minibatch."""
        t = self.torch
        n = int(adv.shape[0])
        arrays = tuple(self._float(x, name) for x, name in ((obs, "obs"), (act, "act"), (old_logp, "old_logp"), (adv, "adv"), (returns, "returns")))
        if arrays[0].numel() * self.lib.tb_act_dim(self.kind) != arrays[1].numel() * self.lib.tb_obs_dim(self.kind) or arrays[0].shape[0] != n \
                or any(int(x.numel()) != n for x in arrays[2:]):
            raise ValueError("update: obs [n, O], act [n, A], old_logp / adv / returns [n] expected")
        flatten_parameters(self.policy)  # (a no-op unless something re-allocated the parameters)
        if self.policy._flat_params is not self.flat:
            self.flat = self.policy._flat_params
        step = self._adopt_optimizer_state()
        done_any = False
        for _ in range(int(n_epochs)):
            perm = t.randperm(n, device=self.device)
            for s in range(0, n, int(batch_size)):
                step += 1
                self.minibatch(arrays, n, perm.data_ptr() + 8 * s, min(int(batch_size), n - s), step, world)
                done_any = True
        for p, (gv, mv, vv) in zip(self.params, self._views):
            st = self.opt.state[p]
            st["step"] = t.tensor(float(step), dtype=st["step"].dtype, device=st["step"].device)
            if done_any:
                p.grad = gv
        if not done_any:
            return {}
        pg, vl, ent = self.stats.tolist()  # the one device-to-host read
        return {"policy_loss": pg, "value_loss": vl, "entropy": ent}
