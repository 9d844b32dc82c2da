"""Time one TRPO update at the training shape in ONE process on ONE collected rollout: the fused form (tennisbot_rl_amd/trpo.py:
tb_ppo_grad, tb_trpo_fvp, tb_trpo_search, critic-only tb_ppo_apply) against a torch-autograd form of the same update -- the
surrogate's gradient by backward, the Fisher-vector product by double backprop of the KL over the same CG rows (the
construction of agent.py:144-167), the same conjugate gradient, the line search one candidate after another with a host read
each (agent.py:109-142), the critic's epochs as torch minibatch Adam on the value loss. Alternating, a device synchronisation on
both sides of every timed region, one warm-up each, then the median of --runs runs each; every run starts from the same policy
and optimiser state. Prints one JSON line (and writes it to --out); exits 1 if the fused update is slower than the torch form.

    python tools/trpo_rate.py [--env SwingRacket-v0] [--num-envs 4096] [--n-steps 104] [--runs 5] [--out profiles/r10_trpo_rate.json]
    python tools/trpo_rate.py --net mlp64 --form sb3 --out profiles/r17_trpo_sb3_rate.json   # sb3_contrib's form on SB3's [64, 64] net

--form sb3: both sides run sb3_contrib's update (tennisbot_rl_amd/trpo.py): its constants, and the acceptance KL < delta and L > L_0,
the torch side measuring L_0 with one more forward pass in front of the search.

    python tools/trpo_rate.py --form agent_returns --out profiles/r18_trpo_returns_rate.json

--form agent_returns: no torch side. One update of the critic-free form beside one of form="agent", both fused, alternating in one
process, and one tb_trpo_returns call beside one tb_ppo_gae call at the same shape (returns_rate). No pass/fail threshold: exits 0.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_update(torch, tr, adv, returns):
    """the update of FusedTRPO.update as torch autograd ops on the same rollout"""
    hp, policy, n = tr.hp, tr.policy, tr.n_steps * tr.num_envs
    obs, act, old_lp = tr.obs_seq.reshape(n, -1), tr._raw_actions.reshape(n, -1), tr.logps.reshape(n)
    adv, returns = adv.reshape(n), returns.reshape(n)
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    theta = [p for k, p in policy.named_parameters() if k == "log_std" or k.startswith("policy_net.") or k.startswith("action_net.")]
    value = [p for k, p in policy.named_parameters() if k.startswith("value_net")]
    flat = lambda ts: torch.cat([x.reshape(-1) for x in ts])  # noqa: E731

    def surrogate():
        _, logp, _ = policy.evaluate(obs, act)
        return ((logp - old_lp).exp() * a).mean()

    def kl_to(old_mean, old_ls, x):  # the KL of agent.py:92-97, as the issue's baseline prescribes
        mean, ls = policy.action_net(policy.policy_net(x)), policy.log_std
        return ((ls - old_ls) + 0.5 * (old_ls.exp() ** 2 + (old_mean - mean) ** 2) / ls.exp() ** 2 - 0.5).sum(1).mean()

    g = flat(torch.autograd.grad(surrogate(), theta)).detach()
    m = max(1, int(hp["cg_state_percent"] * n))
    cg_obs = obs[torch.randperm(n, device=obs.device)[:m]]
    with torch.no_grad():
        cg_mean, all_mean, ls0 = policy.action_net(policy.policy_net(cg_obs)), policy.action_net(policy.policy_net(obs)), policy.log_std.detach().clone()

    def fvp(v):
        grads = flat(torch.autograd.grad(kl_to(cg_mean, ls0, cg_obs), theta, create_graph=True))
        return flat(torch.autograd.grad(grads.dot(v), theta)).detach() + hp["cg_damping"] * v

    # conjugate gradient with the structure and precisions of agent.py:169-191 (x, r, scalars float64; p float32), host-side exit
    p, r = g.clone(), g.double()
    x = torch.zeros_like(r)
    rdotr = r.dot(r)
    for _ in range(int(hp["cg_iterations"])):
        f = fvp(p).double()
        alpha = rdotr / p.double().dot(f)
        x += alpha * p.double()
        r -= alpha * f
        new = r.dot(r)
        p = (r + (new / rdotr) * p.double()).float()
        rdotr = new
        if float(rdotr) < hp["cg_tolerance"]:
            break
    x = x.float()
    step = float((2 * hp["kl_delta"] / x.dot(fvp(x))).sqrt())
    start = flat(theta).detach().clone()
    accepted = -1

    def set_theta(vec):  # in place: the parameters stay views of the trainer's flat vector
        off = 0
        for q in theta:
            q.copy_(vec[off:off + q.numel()].view(q.shape))
            off += q.numel()

    sb3 = getattr(tr, "form", "agent") == "sb3"
    with torch.no_grad():
        L0 = float(surrogate()) if sb3 else 0.0
        for k in range(int(hp["search_candidates"])):
            set_theta(start + step * x)
            kl, L = float(kl_to(all_mean, ls0, obs)), float(surrogate())
            if kl == kl and L == L and abs(kl) != float("inf") and abs(L) != float("inf") and ((kl < hp["kl_delta"] and L > L0) if sb3 else (kl <= hp["kl_delta"] and L >= 0)):
                accepted = k
                break
            step /= hp["search_decay"]
        if accepted < 0:
            set_theta(start)
    opt = torch.optim.Adam(value, lr=hp["learning_rate"], eps=1e-5)
    for _ in range(int(hp["n_epochs"])):
        perm = torch.randperm(n, device=obs.device)
        for s in range(0, n, tr.batch_size):
            idx = perm[s:s + tr.batch_size]
            v = policy.value_net(policy.value_net_body(obs[idx])).squeeze(-1)
            loss = hp["vf_coef"] * ((returns[idx] - v) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(value, hp["max_grad_norm"])
            opt.step()
    return {"accepted_k": accepted, "value_loss": float(loss.detach()) / hp["vf_coef"]}


def returns_rate(args):
    """--form agent_returns: one update of form="agent_returns" (no critic) beside one of form="agent" (GAE, the critic's epochs), each
    on its own trainer's collected rollout at the same shape, alternating in this one process; and the estimators alone, one
    tb_trpo_returns call beside one tb_ppo_gae call (20 calls each, alternating, a synchronisation on both sides). Medians; no
    threshold: the two updates do different work, the figures are what each costs."""
    import torch
    from tennisbot_rl_amd.trpo import TRPOTrainer
    kw = dict(num_envs=args.num_envs, n_steps=args.n_steps, device="cuda:0", seed=0, policy=args.net)
    trainers = {"agent": TRPOTrainer(args.env, form="agent", **kw), "agent_returns": TRPOTrainer(args.env, form="agent_returns", **kw)}
    inputs, start = {}, {}
    for name, tr in trainers.items():
        tr.collect()
        inputs[name] = tr.advantages(tr.last_value)
        start[name] = copy.deepcopy(tr.policy.state_dict()), copy.deepcopy(tr.opt.state_dict())
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, result

    times, stats = {name: [] for name in trainers}, {}
    for k in range(args.runs + 1):            # run 0 of each is the warm-up
        for name, tr in trainers.items():
            tr.policy.load_state_dict(start[name][0]); tr.opt.load_state_dict(copy.deepcopy(start[name][1]))
            s, stats[name] = timed(lambda: tr.update(*inputs[name]))
            if k:
                times[name].append(s)
    estimator = {name: [] for name in trainers}
    for k in range(21):
        for name, tr in trainers.items():
            s, _ = timed(lambda: tr.advantages(tr.last_value))
            if k:
                estimator[name].append(s)
    rows = args.num_envs * args.n_steps
    out = {"tool": "trpo_rate", "env": args.env, "num_envs": args.num_envs, "n_steps": args.n_steps, "net": args.net, "form": "agent_returns", "rows": rows,
           "finished_rows": stats["agent_returns"]["finished_rows"], "finished_share": stats["agent_returns"]["finished_share"], "runs": args.runs,
           "agent_batch_size": trainers["agent"].batch_size, "agent_n_epochs": trainers["agent"].hp["n_epochs"], "device": torch.cuda.get_device_name(0)}
    for name in trainers:
        out[name + "_update_s"] = statistics.median(times[name])
        out[name + "_runs_s"] = [round(s, 6) for s in times[name]]
        out[name + "_last_stats"] = {k: v for k, v in stats[name].items() if v == v}   # (the critic-free form's value_loss is NaN: left out)
    out["tb_trpo_returns_call_s"] = statistics.median(estimator["agent_returns"])
    out["tb_ppo_gae_call_s"] = statistics.median(estimator["agent"])
    out["estimator_calls"] = 20
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for tr in trainers.values():
        tr.env.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="SwingRacket-v0", choices=["SwingRacket-v0", "Tennisbot-v0"])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=104)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--net", default="default", choices=["default", "mlp64"], help="mlp64: SB3's [64, 64] on SwingRacket-v0")
    ap.add_argument("--form", default="agent", choices=["agent", "sb3", "agent_returns"],
                    help="the update both sides run: agent.py's or sb3_contrib's; agent_returns: the critic-free form beside form=agent, both fused, no threshold")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (a median of fewer says little)")
    if args.form == "agent_returns":
        return returns_rate(args)
    import torch
    from tennisbot_rl_amd.trpo import TRPOTrainer
    tr = TRPOTrainer(args.env, num_envs=args.num_envs, n_steps=args.n_steps, device="cuda:0", seed=0, policy=args.net, form=args.form)
    tr.collect()
    adv, returns = tr.advantages(tr.last_value)
    torch.cuda.synchronize()
    start = copy.deepcopy(tr.policy.state_dict()), copy.deepcopy(tr.opt.state_dict())

    def run(fn):
        tr.policy.load_state_dict(start[0]); tr.opt.load_state_dict(copy.deepcopy(start[1]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats

    forms = (("torch", lambda: torch_update(torch, tr, adv, returns)), ("fused", lambda: tr.update(adv, returns)))
    times, stats = {"torch": [], "fused": []}, {}
    for k in range(args.runs + 1):            # run 0 of each is the warm-up
        for name, fn in forms:
            s, stats[name] = run(fn)
            if k:
                times[name].append(s)
    out = {"tool": "trpo_rate", "env": args.env, "num_envs": args.num_envs, "n_steps": args.n_steps, "net": args.net, "form": args.form, "rows": args.num_envs * args.n_steps,
           "cg_rows": int(tr.hp["cg_state_percent"] * args.num_envs * args.n_steps), "batch_size": tr.batch_size, "n_epochs": tr.hp["n_epochs"], "runs": args.runs,
           "device": torch.cuda.get_device_name(0)}
    for name in ("torch", "fused"):
        out[name + "_update_s"] = statistics.median(times[name])
        out[name + "_runs_s"] = [round(s, 6) for s in times[name]]
        out[name + "_last_stats"] = stats[name]
    out["fused_over_torch"] = out["fused_update_s"] / out["torch_update_s"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    tr.env.close()
    return 0 if out["fused_update_s"] <= out["torch_update_s"] else 1


if __name__ == "__main__":
    sys.exit(main())
