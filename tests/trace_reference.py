"""The reference for every frame of tb_swing_trace, from the float32 oracle alone (bit-exact with the HIP path).

The SwingRacket physics never reads step_count; only the termination tests do (swingracket_env.py:105-106, 127-128). So a copy of
an env's pre-step words with its step-count row rewritten ends its step where we want it to:
  row 28 = 800 - k: one oracle step on the copy runs the agent's substep plus exactly k >= 1 flight substeps, then the 800-limit ends
             it; without TB_F_AUTO_RESET the oracle keeps that state, so get_state_words is the full state after substep s = 1 + k;
  row 28 = 0:       the copy runs the agent's substep alone: the state after s = 1.
Only the step-count row of such a copy differs from the traced row's, which is the input step count + s by the trace's contract;
the helper writes that value in. The last sample of an env (s = ns) is the state of the uninterrupted step itself.
"""
import numpy as np

from oracle import OracleBatch
from tennisbot_rl_amd.params import ENV_SWING, F_AUTO_RESET, STATE_WORDS
from tennisbot_rl_amd.stepper import trace_frame_substeps

W = STATE_WORDS[ENV_SWING]
ROW_STEP = W - 2


def n_samples(ns, stride):
    """how many samples the rule takes of a step of ns substeps (n_frames, whether they fit max_frames or not)"""
    return 1 + (ns - 1) // stride + ((ns - 1) % stride != 0)


def swing_fixtures():
    """The four hand-built flights (step_count 25, goal (-6, 1), racket and spawn at (8, 0, 0.6), zero action) and their outcomes on
    the oracle at default parameters: words uint32 [30, 4], done [4], actions [4, 6], and per env (substeps, reward or None, the
    counter that ends it)."""
    from helpers import make_words
    ball_pos = [(-6.0, 1.0, 1.5), (0.0, 3.0, -5.0), (7.9, 0.0, 1.4), (-5.7, 1.0, 0.8)]
    ball_vel = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0)]
    words, done = make_words(ENV_SWING, 4, racket_pos=(8.0, 0.0, 0.6), spawn_pos=(8.0, 0.0, 0.6), goal=(-6.0, 1.0), step_count=25,
                             ball_pos=np.array(ball_pos), ball_vel=np.array(ball_vel))
    outcomes = [(128, 70.0, "goal_hits"), (776, 0.0, "timeouts"), (129, None, "ball_court_terminations"), (88, None, "goal_hits")]
    return words, done, np.zeros((4, 6), np.float32), outcomes


def param_sets():
    """name -> (TbParams, the mixed_batch seed): the parameter sets the trace is checked under. With every seed below the batch holds
    a flight with a racket contact in it and every ending (tests/test_trace_reference.py asserts it on the oracle)."""
    from helpers import draw_engine_params
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_BALL, F_RACKET_GROUND, default_params, reference_rolling_friction
    return {
        "default": (default_params(), 1),
        "net_off": (default_params(flags=F_RACKET_BALL), 1),
        "racket_ground_rolling": (default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction()), 1),   # the RG instantiation
        "magnus_spin": (default_params(magnus_k=5e-4, ball_spin_max=200.0), 1),
        "draw_a": (default_params(**draw_engine_params(np.random.default_rng(11))), 1),
        "draw_b": (default_params(flags=F_DEFAULT | F_RACKET_GROUND, **draw_engine_params(np.random.default_rng(12), rolling=True)), 1),
    }


def touching_row(params, step_count):
    """a non-flight row whose one substep has a racket<->ball contact: the ball 2 mm inside the racket face's contact distance at the
    racket's COM, moving into it at 1 m/s. The bonus of swingracket_env.py:98-101 is paid while the new step count is below 25."""
    from helpers import make_words
    x = 8.0 + params.racket_half_thick + params.hull_margin + params.ball_radius - 0.002
    return make_words(ENV_SWING, 1, racket_pos=(8.0, 0.0, 0.6), spawn_pos=(8.0, 0.0, 0.6), goal=(-6.0, 1.0), step_count=step_count,
                      ball_pos=(x, 0.0, 0.6), ball_vel=(-1.0, 0.0, 0.0))[0][:, 0]


def mixed_batch(params, seed, n=130):
    """n pre-step rows for one wave and more, flights and non-flights mixed: the four fixtures; states after 25 random steps of the
    oracle's own episodes (racket contacts during the swing included), whose next step is the flight; the same episodes after 0, 10
    and 24 steps and three hand-built rows with the ball on the racket at those step counts (one substep, no flight, the contact
    bonus where it is due); and two step-25 states entering with a non-zero done byte (1: a restoring force still pending, 2: none).
    Actions are uniform in [-1, 1), the hand-built rows' zero. A prefix
    of the batch is a mixed batch too: row 0 is a flight, rows 0 .. 4 hold a flight, a non-flight, the 776-substep flight and a done
    row. Returns (words uint32 [30, n], done uint8 [n], actions float32 [n, 6])."""
    p = params.copy()
    p.flags &= ~F_AUTO_RESET
    rng = np.random.default_rng(seed)
    b = OracleBatch(p, ENV_SWING, n, seed=seed, precision="f32")
    b.reset()
    snap = {}
    for t in range(26):
        if t in (0, 10, 24, 25):
            snap[t] = b.get_state_words()[0].copy()
        if t < 25:
            b.step(rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32))
    b.close()
    fw, _, _, _ = swing_fixtures()
    words = np.zeros((W, n), np.uint32)
    done = np.zeros(n, np.uint8)
    actions = rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32)
    head = [("fix", 0), ("touch", 10), ("fix", 1), ("done1", 1), ("fix", 2), ("fix", 3), (0, 2), (24, 3), ("done2", 4), ("touch", 0),
            ("touch", 24), (10, 5)]
    for r in range(n):
        what, j = head[r] if r < len(head) else ((0, 10, 24)[(r // 8) % 3] if r % 8 == 5 else 25, r)
        if what == "fix":
            words[:, r] = fw[:, j]
            actions[r] = 0.0
        elif what == "touch":
            words[:, r] = touching_row(p, j)
            actions[r] = 0.0
        elif what in ("done1", "done2"):
            words[:, r] = snap[25][:, j]
            done[r] = 1 if what == "done1" else 2
        else:
            words[:, r] = snap[what][:, j]
    return words, done, actions


class TraceOracle:
    """One batch of pre-step states and the oracle's account of its step: the uninterrupted step once, any intermediate state on
    request (computed in batches, each (env, substep) once)."""

    def __init__(self, params, words, done, actions, threads=1):
        self.params = params.copy()
        self.params.flags &= ~F_AUTO_RESET   # the oracle keeps the terminal state; the trace never resets either
        self.words = np.ascontiguousarray(words, np.uint32).reshape(W, -1).copy()
        self.n = self.words.shape[1]
        self.done_in = np.zeros(self.n, np.uint8) if done is None else np.ascontiguousarray(done, np.uint8).copy()
        self.actions = np.ascontiguousarray(actions, np.float32).reshape(self.n, 6).copy()
        self.threads = threads
        self.step0 = self.words[ROW_STEP].view(np.int32).copy()
        full = self._step(self.words, self.done_in, self.actions)
        self.obs, self.reward, self.done, self.substeps, self.final, self.counters = full
        self._cache = {}

    def _step(self, words, done, actions):
        b = OracleBatch(self.params, ENV_SWING, words.shape[1], precision="f32", threads=self.threads)
        b.set_state_words(words, done)
        obs, rew, d, sub = b.step(actions)
        w, _ = b.get_state_words()
        c = np.array([int(x) for x in b.counters()], np.int64)
        b.close()
        return obs, rew, d, sub, w, c

    def _cut_words(self, pairs):
        """the copies that end after substep s of env i, for (i, s) pairs with s < ns[i]"""
        idx = np.array([i for i, _ in pairs], np.int64)
        w = self.words[:, idx].copy()
        w[ROW_STEP] = np.array([0 if s == 1 else 800 - (s - 1) for _, s in pairs], np.int32).view(np.uint32)
        return idx, w

    def _fill(self, pairs):
        todo = sorted(set(p for p in pairs if p not in self._cache))
        if not todo:
            return
        for i, s in todo:
            assert 1 <= s < self.substeps[i] and self.done_in[i] == 0, (i, s)   # only a flight has states before its last
        idx, w = self._cut_words(todo)
        _, _, _, sub, out, _ = self._step(w, np.zeros(len(todo), np.uint8), self.actions[idx])
        assert np.array_equal(sub, np.array([s for _, s in todo], np.int32)), "a cut copy did not stop where it was cut"
        for k, (i, s) in enumerate(todo):
            self._cache[(i, s)] = out[:, k].copy()

    def state_after(self, i, s):
        """the 30 state words of env i after substep s of its step, the step-count word as the trace reports it"""
        ns = int(self.substeps[i])
        assert 1 <= s <= ns
        if s == ns:
            row = self.final[:, i].copy()
        else:
            self._fill([(i, s)])
            row = self._cache[(i, s)].copy()
        row[ROW_STEP] = np.array([self.step0[i] + s], np.int32).view(np.uint32)[0]
        return row

    def frames(self, stride, max_frames):
        """what tb_swing_trace stores: (frames uint32 [max_frames, 30, n], n_frames int32 [n], the substep number of every row
        int32 [max_frames, n])"""
        steps = np.array([trace_frame_substeps(int(ns), stride, max_frames) for ns in self.substeps], np.int32).T
        self._fill([(i, int(s)) for i in range(self.n) for s in steps[:, i] if s < self.substeps[i]])
        fr = np.zeros((max_frames, W, self.n), np.uint32)
        for i in range(self.n):
            for k in range(max_frames):
                fr[k, :, i] = self.state_after(i, int(steps[k, i]))
        nf = np.array([n_samples(int(ns), stride) for ns in self.substeps], np.int32)
        return fr, nf, steps

    def flight_contact_substeps(self):
        """racket<->ball contact substeps (counter 0) inside the flights, the agent's substep not counted: the whole step's count
        minus the count of the first substeps alone"""
        fl = [i for i in range(self.n) if self.substeps[i] > 1]
        if not fl:
            return 0
        idx, w = self._cut_words([(i, 1) for i in fl])
        first = self._step(w, np.zeros(len(fl), np.uint8), self.actions[idx])[5]
        rest = [i for i in range(self.n) if self.substeps[i] == 1]
        alone = self._step(self.words[:, rest], self.done_in[rest], self.actions[rest])[5][0] if rest else 0
        return int(self.counters[0] - first[0] - alone)
