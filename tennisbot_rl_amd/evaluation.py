"""Whole-episode evaluation beside training, and the schedule that keeps the best model.

Counterpart of the two callbacks the reference's scripts install around `learn()` (train_swing.py:111-119, train.py:138-146):
`EvalCallback(eval_freq, deterministic=False, best_model_save_path)` and `CheckpointCallback(save_freq, save_path, name_prefix)`.

  * `PolicyEvaluator` owns a SEPARATE env batch and runs every env's whole episode in one launch (BatchedEnv.policy_evaluate,
    tb_policy_evaluate): the mean is a mean over finished episodes, each counted once from its first step to its first `done`;
    the training batch, its episode phase and its captured graph are never touched, and no torch RNG is drawn from (the
    exploration noise is keyed inside the kernel).
  * `ActorEvaluator` is its counterpart for SAC / TQC: the flat actor vector the learner trains, inside the episode loop of one
    launch (BatchedEnv.sac_evaluate, tb_sac_evaluate).
  * `evaluate_actor_episodes` is the same protocol for a torch actor stepped between env steps (SAC / TQC's default form):
    first-`done` masks and float64 sums stay on the device.
  * `EvalSchedule` fires evaluations and checkpoints as `num_timesteps` crosses multiples of `eval_freq` / `save_freq`.
"""
import math
import os

from .params import ENV_SWING, NET_DEFAULT
from .stepper import ENV_IDS, BatchedEnv

EVAL_ENV_ID_BASE = 1 << 40   # global env ids of evaluation batches: far above any training batch's (rank * num_envs)
BEST_MODEL = "best_model.pt"


def summarise(torch, returns, lengths):
    """{episodes, mean, std, min, max, mean_length} of float64 returns / integer lengths on the device; ONE host read.
    std is the population standard deviation (numpy's default, what SB3's evaluate_policy reports)."""
    r = returns.double()
    row = torch.stack([r.mean(), r.std(unbiased=False), r.min(), r.max(), lengths.double().mean()]).tolist()
    return {"episodes": int(r.numel()), "mean": row[0], "std": row[1], "min": row[2], "max": row[3], "mean_length": row[4]}


class _EpisodeEvaluator:
    """n_envs evaluation envs of their own; a subclass says which launch runs their episodes (_launch)"""

    def __init__(self, kind, n_envs, seed, params, options, device, env_id_base):
        if isinstance(kind, str):
            kind = ENV_IDS[kind]
        self.kind, self.n_envs, self.seed = kind, int(n_envs), int(seed)
        # SwingRacket: the 26th step's fast-forward runs on the pipeline's kernels (tb_policy_evaluate / tb_sac_evaluate require it)
        self.env = BatchedEnv(kind, self.n_envs, device=device, seed=self.seed, env_id_base=int(env_id_base), params=params, track_terminal_obs=False,
                              pipeline=kind == ENV_SWING, options=options)
        self.device = self.env.device
        self.noise_seed = (self.seed * 1000003 + 0x45564C) & 0xFFFFFFFFFFFFFFFF

    def set_racket_scale(self, scale):
        """Tennisbot's racket-size curriculum: takes effect at the reset every evaluation call starts with"""
        self.env.set_racket_scale(float(scale))

    def episodes(self, weights, n_episodes, deterministic=False):
        """(returns float64 [n_episodes], lengths int32 [n_episodes]) on the device: ceil(n_episodes / n_envs) launches, every one
        the next episode of every env; the surplus of the last launch is dropped"""
        n_episodes = int(n_episodes)
        if n_episodes < 1:
            raise ValueError("n_episodes must be >= 1")
        torch = self.env.torch
        rets, lens = [], []
        for _ in range(-(-n_episodes // self.n_envs)):
            r, ln = self._launch(weights, deterministic)
            rets.append(r); lens.append(ln)
        return torch.cat(rets)[:n_episodes], torch.cat(lens)[:n_episodes]

    def evaluate(self, weights, n_episodes, deterministic=False):
        """{episodes, mean, std, min, max, mean_length} over n_episodes whole episodes; float64 on the device, one host read"""
        r, ln = self.episodes(weights, n_episodes, deterministic)
        return summarise(self.env.torch, r, ln)

    def close(self):
        self.env.close()


class PolicyEvaluator(_EpisodeEvaluator):
    """n_envs evaluation envs of their own for the fused policy networks (PPO / TRPO; NET_DEFAULT, Tennisbot's NET_TUNED or SwingRacket's NET_MLP64); weights:
    the packed blob of ppo.pack_policy"""

    def __init__(self, kind, n_envs=64, seed=0, params=None, options=None, device=None, net=NET_DEFAULT, env_id_base=EVAL_ENV_ID_BASE):
        from .stepper import check_net
        self.net = check_net(kind, net)
        super().__init__(kind, n_envs, seed, params, options, device, env_id_base)

    def _launch(self, packed_weights, deterministic):
        return self.env.policy_evaluate(packed_weights, seed=self.noise_seed, deterministic=deterministic, net=self.net)


class ActorEvaluator(_EpisodeEvaluator):
    """the same for the SAC / TQC actor (the two share it); weights: the flat TB_SAC_ACTOR vector -- what the learner's kernels
    train, so there is nothing to pack"""

    def __init__(self, kind, n_envs=64, seed=0, params=None, options=None, device=None, env_id_base=EVAL_ENV_ID_BASE):
        super().__init__(kind, n_envs, seed, params, options, device, env_id_base)

    def _launch(self, actor_flat, deterministic):
        return self.env.sac_evaluate(actor_flat, seed=self.noise_seed, deterministic=deterministic)


def evaluate_actor_episodes(env, act, n_episodes, check_every=8):
    """Whole episodes of a torch actor on `env` (a BatchedEnv with auto_reset and without the pipeline, NOT the training batch):
    reset, then step every env with act(obs) until each has finished its first episode; ceil(n_episodes / num_envs) such rounds.
    Only an env's rewards through its first `done` count. Returns summarise()'s dict."""
    torch, n = env.torch, env.num_envs
    n_episodes = int(n_episodes)
    if n_episodes < 1:
        raise ValueError("n_episodes must be >= 1")
    t_max = 26 if env.kind == ENV_SWING else 1001
    rets, lens = [], []
    with torch.no_grad():
        for _ in range(-(-n_episodes // n)):
            obs = env.reset()
            ret = torch.zeros(n, dtype=torch.float64, device=env.device)
            length = torch.zeros(n, dtype=torch.int32, device=env.device)
            active = torch.ones(n, dtype=torch.bool, device=env.device)
            for t in range(t_max):
                obs, r, d = env.step(act(obs).contiguous())
                ret += torch.where(active, r.double(), torch.zeros_like(ret))
                length += active.int()
                active &= d == 0
                # (SwingRacket: exactly 26 steps, nothing to ask; Tennisbot: a host read every few steps ends the round early)
                if env.kind != ENV_SWING and (t + 1) % check_every == 0 and not bool(active.any()):
                    break
            rets.append(ret); lens.append(length)
    return summarise(torch, torch.cat(rets)[:n_episodes], torch.cat(lens)[:n_episodes])


class EvalSchedule:
    """When to evaluate, what to keep. after_rollout(trainer) is called by the trainers' learn() after every update (SAC / TQC:
    after every vector step); `trainer` needs num_timesteps, rank, evaluate_episodes(n, deterministic) and save(path).
    An evaluation fires when num_timesteps has crossed a multiple of eval_freq since the previous call -- ONE evaluation, however
    many multiples one rollout of thousands of envs crossed -- and likewise a checkpoint at save_freq; 0 switches either off.
    best_model.pt is written (trainer.save) when the mean return strictly exceeds the best so far. Only rank 0 evaluates and
    writes. `history`: one {timesteps, mean, std, mean_length, episodes} row per evaluation."""

    def __init__(self, eval_freq=0, n_eval_episodes=64, deterministic=False, best_model_save_path=None, save_freq=0, save_path=None,
                 name_prefix="rl_model", log=None):
        self.eval_freq, self.save_freq = int(eval_freq), int(save_freq)
        if self.eval_freq < 0 or self.save_freq < 0 or int(n_eval_episodes) < 1:
            raise ValueError("EvalSchedule: eval_freq and save_freq must be >= 0 and n_eval_episodes >= 1")
        if self.save_freq and save_path is None:
            raise ValueError("EvalSchedule: save_freq needs a save_path")
        self.n_eval_episodes, self.deterministic = int(n_eval_episodes), bool(deterministic)
        self.best_model_save_path, self.save_path, self.name_prefix, self.log = best_model_save_path, save_path, name_prefix, log
        self.best_mean = -math.inf
        self.history, self.checkpoints = [], []
        self._seen = 0   # num_timesteps at the previous call

    def reset(self, num_timesteps):
        """start counting crossings from here (a resumed run: call once after trainer.load)"""
        self._seen = int(num_timesteps)

    def best_model_path(self):
        return None if self.best_model_save_path is None else os.path.join(self.best_model_save_path, BEST_MODEL)

    def checkpoint_path(self, num_timesteps):
        return os.path.join(self.save_path, "%s_%d_steps.pt" % (self.name_prefix, int(num_timesteps)))

    def after_rollout(self, trainer):
        now, before = int(trainer.num_timesteps), self._seen
        self._seen = now
        if getattr(trainer, "rank", 0) != 0:
            return None
        result = None
        if self.eval_freq and now // self.eval_freq > before // self.eval_freq:
            result = trainer.evaluate_episodes(self.n_eval_episodes, deterministic=self.deterministic)
            self.history.append({"timesteps": now, "mean": result["mean"], "std": result["std"], "mean_length": result["mean_length"],
                                 "episodes": result["episodes"]})
            improved = result["mean"] > self.best_mean
            if improved:
                self.best_mean = result["mean"]
                if self.best_model_save_path is not None:
                    os.makedirs(self.best_model_save_path, exist_ok=True)
                    trainer.save(self.best_model_path())
            if self.log:
                self.log("eval at %d timesteps: %d episodes, mean return %.3f +- %.3f, mean length %.1f%s"
                         % (now, result["episodes"], result["mean"], result["std"], result["mean_length"], "  (new best)" if improved else ""))
        if self.save_freq and now // self.save_freq > before // self.save_freq:
            os.makedirs(self.save_path, exist_ok=True)
            path = self.checkpoint_path(now)
            trainer.save(path)
            self.checkpoints.append(path)
        return result


# ------------------------------------------------------------------------------------------------ the training scripts' share
def add_schedule_arguments(ap):
    """--eval-freq / --n-eval-episodes / --eval-deterministic / --save-freq: all off by default"""
    ap.add_argument("--eval-freq", type=float, default=0, help="evaluate whole episodes on a separate env batch every this many timesteps and keep "
                    "the best model as best_model.pt beside --save (the reference's EvalCallback); 0: off")
    ap.add_argument("--n-eval-episodes", type=int, default=64, help="episodes per evaluation")
    ap.add_argument("--eval-deterministic", action="store_true", help="evaluate the mean action (the reference evaluates the stochastic policy)")
    ap.add_argument("--save-freq", type=float, default=0, help="checkpoint every this many timesteps as rl_model_<timesteps>_steps.pt beside --save "
                    "(the reference's CheckpointCallback); 0: off")


def model_dir(save_path):
    """the directory best models and periodic checkpoints go to: that of --save"""
    return os.path.dirname(os.path.abspath(save_path))


def resolve_load(load, save_path):
    """--load best -> best_model.pt in the directory of --save; any other value is a path and is returned as it is"""
    if load == "best":
        return os.path.join(model_dir(save_path), BEST_MODEL)
    return load


def schedule_from_args(args, save_path, log=print):
    """the EvalSchedule of a script's arguments, or None when neither --eval-freq nor --save-freq is given"""
    if not (args.eval_freq or args.save_freq):
        return None
    d = model_dir(save_path)
    return EvalSchedule(eval_freq=int(args.eval_freq), n_eval_episodes=args.n_eval_episodes, deterministic=args.eval_deterministic, best_model_save_path=d,
                        save_freq=int(args.save_freq), save_path=d, log=log)
