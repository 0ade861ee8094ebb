"""Randomised engine lives: the schedule generator and the runner that replays a
schedule on the oracle (and, given engines, on them too, comparing every output
bit for bit). Pure numpy: no engine import; tests/test_gpu_life_fuzz.py passes
the engines and the binding module in, tests/test_life_schedule_cpu.py passes
none and replays on the oracle alone.

A schedule is a dict: the shape and engine arguments, the initial option
assignment and a list of steps (dicts with an "op"):
  rounds (c sim rounds in one run_rounds call) / replay (one replay_round_errs
  round), each followed by the update stream's comparison over one of three
  routes; the disturbances register, register_batch, set_valid, add,
  materialize, reinit, options, write; and observe steps. A validity flip and a
  kernel 2 -> 1 -> 2 switch are two calls 1-3 rounds apart (the second carries
  "tail"); they count as one disturbance.
Phase 1 (the first two thirds of the rounds) holds only disturbances that keep
RecordFacts::c_monotone (round_plan.h): no neutral vote, no write_records, no
replay, no warm_skip = 0. In an honest seed the phase-1 disturbances start
after round 6 and lie at least 5 rounds apart, so that the network is settled
again before each one. In a *taken* seed (honest, k = 8) the rounds flagged
"taken" are the round just before each phase-1 disturbance and one more; there
the deferring engine must move fewer bytes than its plain twin. Seeds with
k < 8 plan none of the deferred forms (plan_round asks k == 8 for vv, klazy,
reference and uniform rows) and Byzantine seeds never settle, so neither
carries taken rounds.

Lossy lives (make_lossy_schedule, N_LOSSY_SEEDS of them; rule R5) are lives of
the same kind, drawn from a generator of their own, with loss laid over them.
Their seed mix is lossy_config's: k = 12 once, k in {1, 3, 5} three times, three
Byzantine seeds, the rest honest at k = 8. Three more ops:
  set_loss (thr, mode) / set_responding (nodes, responds): av_set_loss and
  av_set_responding on every engine; observe with what = "lost": av_sample_lost
  of the round about to run against lossy_ref.lost_table, and av_lost_responses.
While the threshold is non-zero or a node is down, Life runs each sim round
through lossy_ref.LossyRef.round instead of Sim.run_round; a replay round is
the plain one whatever the loss state and loses nothing.
The overlay (_overlay) lays one to three stretches [a, b) of 2-8 rounds, at
least 3 rounds apart, over the schedule. A stretch opens before round a, ahead
of that round's disturbances, with set_loss and/or set_responding(.., 0), and
closes before round b with set_loss(0) and set_responding(.., 1). Modes and
probabilities: SKIP {0.10, 0.25, 0.60}, NEUTRAL {0.05, 0.15}; with nodes down
the threshold is sometimes 0; one seed's first stretch has threshold 2^32 - 1.
Down sets by (seed + stretch) mod 4: none, a few nodes, nodes 0 and n - 1, one
whole 32-node word of the bitset; one seed's first stretch starts with one
round of every node down. A stretch of 3 rounds or more may change part-way:
SKIP <-> NEUTRAL, a node back up, one more down. A stretch that starts in
phase 1 is SKIP throughout (a NEUTRAL round clears c_monotone). Each stretch is
laid over a disturbance of the kind WANTED names for it (or the replay round)
where the life has one, else late in the life, where records finalize. rounds
steps are cut at every stretch edge and change and keep their route and digest
range. A taken flag is cleared in [a, b + 2): a lossy round defers nothing, and
the plain round after it runs in the check form and only sets warm_all again.
In a taken seed the first stretch is, where the life has room for one, a phase-1
SKIP stretch ending at a b with no disturbance in b - 2 .. b + 2 (no re-init in
b - 9 .. b) and c_monotone kept through b + 2; if the options then in force let plan_round defer (kernel 2
and virtual_votes, or count_lazy with count_bound < 120), round b + 2 runs as a
step of its own, flagged taken and "regain": the engine must be deferring
again. tests/test_life_schedule_cpu.py checks on the oracle that rows are
identical and targets valid at b, b + 1 and b + 2."""
import numpy as np

from census_ref import census_from_words
from lossy_ref import LossyRef, lost_table

N_SEEDS = 32
INIT_ACCEPTED, INIT_BERNOULLI, INIT_PAIRS = 2, 3, 4
P97, P80 = int(0.97 * 2**32), int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)
ENC_BUCKETS_DEFAULT = 1 << 26
LOG_CAPACITY = 1 << 20

# N x M: the smallest shapes at which each layout rule binds (a tile is 64 lanes, BL = ceil(M / 32))
SHAPES = [(64, 33), (96, 100), (200, 256), (67, 640), (130, 1000), (48, 1100)]
INITS = [(INIT_ACCEPTED, 0), (INIT_BERNOULLI, P97), (INIT_BERNOULLI, P80), (INIT_PAIRS, 0)]
DEFERRALS = ("virtual_votes", "count_lazy", "uniform_rows", "quiet_tiles")
DEFAULTS = {"virtual_votes": 1, "count_lazy": 1, "uniform_rows": 1, "quiet_tiles": 1, "kernel": 2}
PHASE1_KINDS = ("register", "register_batch", "set_valid", "add", "materialize", "reinit", "options", "options",
                "kernel_flip")
PHASE2_KINDS = PHASE1_KINDS + ("neutral", "write", "write", "neutral")
OBSERVATIONS = ("read_full", "read_rect", "cells", "invs", "pref", "census", "live")
NO_ERRS = np.array([0, 0, 0, 1], np.uint32)
ALL_ERRS = np.array([0, 0, 0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)

# the plain twin: kernel 2 with every deferral and shortcut option off. warm_skip stays on: it is the
# invariant that lets the twin run the same warm kernel build, so a byte difference is a deferral's.
PLAIN_OPTIONS = [("kernel", 2), ("virtual_votes", 0), ("count_lazy", 0), ("k_hi_virtual", 0), ("uniform_rows", 0),
                 ("ref_rows", 0), ("quiet_tiles", 0), ("uni_votes", 0), ("uni_merge", 1), ("settled_fast", 0),
                 ("settled_lean", 0), ("wave_runs", 0), ("tile_draw", 0), ("wave_dense", 0), ("dropin_fast", 0),
                 ("fresh", 0)]


def option_values(k):
    """Every result-preserving option value of the issue's list (warm_skip and fresh: switch-off only)."""
    return {
        "virtual_votes": [0, 1], "vv_min_bl": [1, 8, 33], "count_lazy": [0, 1], "k_hi_virtual": [0, 1],
        "uniform_rows": [0, 1], "ref_rows": [0, 1], "quiet_tiles": [0, 1], "uni_votes": [0, 1], "uni_merge": [1, 2, 8],
        "settled_fast": [0, 1], "settled_lean": [0, 1], "wave_runs": [0, 1], "sweep_nopipe": [0, 1], "tile_draw": [0, 1],
        "materialize_run": [1, 4, 64], "plane_nt": [0, 1], "store_policy": [0, 1, 2, 3], "wave_dense": [0, 1, 8, 64],
        "dense_min": [1, 2, 6, 32 * k + 1], "dropin_fast": [0, 1], "enc_buckets": [1, 7, ENC_BUCKETS_DEFAULT],
        "kernel": [1, 2], "fresh": [0], "warm_skip": [0], "sweep_blocks": [-1, -2, 0, 1, 3],
        "tiles_per_wave": [0, 1, 4, 16],
    }


def seed_config(seed):
    """Shape, k and Byzantine share of a seed: one seed in four Byzantine, one in eight k in {3, 5}."""
    n, m = SHAPES[(seed + seed // 4) % len(SHAPES)]
    return n, m, (BYZ20 if seed % 4 == 3 else 0), seed % 8 == 5


class _Gen:
    def __init__(self, seed, rng=None, config=None):
        """rng, config = (n, m, byz, k): the lossy lives' own generator and seed mix."""
        self.rng = rng = np.random.default_rng(0x11FE0000 + seed) if rng is None else rng
        if config is None:
            self.n, self.m, self.byz, small_k = seed_config(seed)
            self.k = int(rng.choice([3, 5])) if small_k else 8
        else:
            self.n, self.m, self.byz, self.k = config
        self.taken_seed = self.byz == 0 and self.k == 8
        self.values = option_values(self.k)
        self.off_used = set()
        self.current = dict(DEFAULTS)

    def draw_options(self, phase2, fixed=()):
        """Random values for 1-3 option names; fixed: (name, value) pairs that are part of the draw."""
        rng = self.rng
        names = [nm for nm in self.values if nm not in self.off_used]
        if not phase2 and "warm_skip" in names:
            names.remove("warm_skip")  # clears c_monotone: phase 2 only
        fixed = dict(fixed)
        size = max(len(fixed), int(rng.integers(1, 4)))
        free = [nm for nm in names if nm not in fixed]
        picked = list(fixed) + [free[i] for i in rng.choice(len(free), size=size - len(fixed), replace=False)]
        out = []
        for nm in sorted(picked, key=names.index):
            v = fixed[nm] if nm in fixed else int(rng.choice(self.values[nm]))
            if nm in ("fresh", "warm_skip"):
                self.off_used.add(nm)
            if nm in self.current:
                self.current[nm] = v
            out.append((nm, v))
        return out

    def deferring(self):
        c = self.current
        return c["kernel"] == 2 and any(c[d] for d in DEFERRALS)

    def votes(self, errs_from, lo, hi):
        rng = self.rng
        size = int(rng.integers(lo, hi))
        ts = rng.integers(-3, self.m + 3, size=size)
        if size > 3:  # duplicates inside one Response
            ts[rng.random(size) < 0.25] = int(rng.integers(0, self.m))
        return ts.astype(np.int64), rng.choice(errs_from, size).astype(np.uint32)

    def disturbance(self, kind, phase2):
        """The step(s) of one disturbance: [(round offset, step)]."""
        rng, n, m = self.rng, self.n, self.m
        if kind in ("register", "neutral"):
            ts, errs = self.votes(ALL_ERRS if kind == "neutral" else NO_ERRS, 1, 20)
            if kind == "neutral":
                errs[int(rng.integers(0, errs.size))] = ALL_ERRS[6 + int(rng.integers(0, 2))]
            return [(0, dict(op="register", node=int(rng.integers(0, n)), targets=ts, errs=errs))]
        if kind == "register_batch":
            n_resp = int(rng.integers(2, 7))
            parts = [self.votes(NO_ERRS, 0, 12) for _ in range(n_resp)]
            if rng.random() < 0.5:  # every Response ascending and duplicate-free: the batch fast path
                parts = [(np.unique(t), e[:np.unique(t).size]) for t, e in parts]
            return [(0, dict(op="register_batch", nodes=rng.integers(0, n, size=n_resp).astype(np.int64),
                             offsets=np.concatenate([[0], np.cumsum([len(t) for t, _ in parts])]).astype(np.int64),
                             targets=np.concatenate([t for t, _ in parts]).astype(np.int64),
                             errs=np.concatenate([e for _, e in parts]).astype(np.uint32)))]
        if kind == "set_valid":
            t = int(rng.integers(0, m)) if rng.random() < 0.7 else m - 1
            return [(0, dict(op="set_valid", t=t, valid=False)),
                    (int(rng.integers(1, 4)), dict(op="set_valid", t=t, valid=True, tail=True))]
        if kind == "kernel_flip":  # kernel 2 -> 1 -> 2 in mid-life: the first-generation kernel reads no deferred form
            self.current["kernel"] = 2
            return [(0, dict(op="options", set=[("kernel", 1)])),
                    (int(rng.integers(1, 4)), dict(op="options", set=[("kernel", 2)], tail=True))]
        if kind == "add":
            size = int(rng.integers(1, 11))
            return [(0, dict(op="add", node=int(rng.integers(0, n)), targets=rng.integers(0, m, size=size).astype(np.int64),
                             accepted=rng.integers(0, 2, size=size).astype(np.uint8)))]
        if kind == "materialize":
            return [(0, dict(op="materialize"))]
        if kind == "reinit":
            return [(0, dict(op="reinit"))]
        if kind == "options":
            return [(0, dict(op="options", set=self.draw_options(phase2)))]
        assert kind == "write"
        h, w = int(rng.integers(1, min(n, 40) + 1)), int(rng.integers(1, min(m, 90) + 1))
        n0, t0 = int(rng.integers(0, n - h + 1)), int(rng.integers(0, m - w + 1))
        cons = rng.integers(0, 256, size=(h, w)).astype(np.uint32)
        votes = rng.integers(0, 256, size=(h, w)).astype(np.uint32) & cons
        count = rng.integers(0, 128, size=(h, w)).astype(np.uint32)
        count[rng.random((h, w)) < 0.15] = 127
        acc = rng.integers(0, 2, size=(h, w)).astype(np.uint32)
        words = votes | (cons << 8) | (((count << 1) | acc) << 16)
        gone = rng.random((h, w)) < 0.2  # count >= 128: no record; canonical or with stray low bits
        words[gone] = (0xFFFE0000 | (acc[gone] << 16)) ^ np.where(rng.random(int(gone.sum())) < 0.5, 0,
                                                                  rng.integers(0, 1 << 16, int(gone.sum()))).astype(np.uint32)
        return [(0, dict(op="write", n0=n0, t0=t0, words=words.astype(np.uint32)))]

    def observation(self):
        rng, n, m = self.rng, self.n, self.m
        what = str(rng.choice(OBSERVATIONS))
        ob = dict(op="observe", what=what)
        if what in ("read_rect", "invs", "census"):
            a, b = sorted(rng.integers(0, n + 1, size=2).tolist())
            whole = what == "census" and rng.random() >= 0.5  # half the censuses count every node
            n0, n1 = (0, n) if whole or a == n else (a, max(b, a + 1))
            ob.update(n0=n0, n1=n1)
        if what == "read_rect":  # a rectangle not aligned to the 32-target blocks
            a, b = sorted(rng.integers(0, m + 1, size=2).tolist())
            t0 = min(a, m - 1)
            ob.update(t0=t0, t1=max(b, t0 + 1))
        if what == "cells":
            ob.update(cells=[(int(rng.integers(0, n)), int(rng.integers(0, m))) for _ in range(8)])
        if what in ("census", "live"):
            ob.update(honest_only=bool(rng.integers(0, 2)))
        return ob


def make_schedule(seed):
    return _build(_Gen(seed), seed, 7000 + seed)[0]


def _build(g, seed, engine_seed):
    """The schedule of generator g, and what the lossy overlay needs to know of it: the disturbance
    steps per round, their kinds [(round, kind)] and the replay round."""
    rng, n, m, k = g.rng, g.n, g.m, g.k
    # INIT_PAIRS starts every target at an even split, which an honest network of these sizes leaves only
    # after 9-24 rounds: too late for settled stretches inside phase 1, so the taken seeds draw the others
    init_mode, init_param = INITS[int(rng.integers(0, len(INITS) - (1 if g.taken_seed else 0)))]
    rounds = int(rng.integers(36, 49))
    phase1 = 2 * rounds // 3
    # the initial assignments of the 32 seeds together hold every listed value of the options that may
    # be set at any time (the switch-off-only names come up in the re-draws)
    flat = [(nm, v) for nm, vs in g.values.items() for v in vs if nm not in ("fresh", "warm_skip")]
    initial = g.draw_options(False, fixed=[flat[i] for i in (seed % N_SEEDS, seed % N_SEEDS + N_SEEDS) if i < len(flat)])

    at = {}  # round index -> disturbance steps run before that round
    kinds = []  # (round, kind) of every disturbance
    alone = set()  # rounds that run as a step of their own (the taken rounds)
    taken = {}  # taken round -> the deferral options on in that round

    def place(r, kind, phase2):
        last = r
        kinds.append((r, kind))
        for off, step in g.disturbance(kind, phase2):
            rr = min(r + off, rounds - 1)
            at.setdefault(rr, []).append(step)
            last = max(last, rr)
        return last

    # RecordFacts::count_bound (round_plan.h) as the engine will keep it, at the start of round bound_r:
    # count steps are deferred only while it is < 120
    bound, bound_r = -6, 0

    def bound_at(x):
        return min(127, bound + 8 * (x - bound_r))

    # phase 1
    first = True
    # Bernoulli(0.8) rows agree from round 6 at the latest (Bernoulli(0.97): 3), and the extra taken round
    # before the first disturbance needs the three rounds before it settled
    spaced = g.byz == 0  # honest seeds: no disturbance before round 6, >= 5 rounds between them
    r = int(rng.integers(10, 13)) if spaced else int(rng.integers(1, 4))
    while r < phase1:
        kind = str(rng.choice(PHASE1_KINDS))
        if g.taken_seed:
            if g.deferring():
                on = [d for d in DEFERRALS if g.current[d]]
                taken[r - 1] = on
                if first:  # one more taken round, after round 6, inside the first settled stretch
                    taken[r - 2] = on
                    first = False
            alone.update((r - 1, r - 2))
        last = place(r, kind, False)
        if kind == "reinit":
            bound, bound_r = -6, r
        elif kind in ("register", "register_batch"):
            bound, bound_r = min(127, bound_at(r) + max_node_votes(at[r][-1])), r
        # Past count_bound 120 (16 rounds after an init, sooner after drop-in votes) no count step is
        # deferred, and quiescent tiles are such steps; with virtual_votes off nothing would be left to
        # disturb before the next disturbance (at most 7 rounds on), so the records are re-initialised too
        if g.taken_seed and kind != "reinit" and not g.current["virtual_votes"] and bound_at(last + 6) >= 120:
            at[r].append(dict(op="reinit"))
            kinds.append((r, "reinit"))
            kind, bound, bound_r = "reinit", -6, r
        # a re-initialised network converges anew first
        r = last + (int(rng.integers(5, 8)) + (5 if kind == "reinit" else 0) if spaced else int(rng.integers(1, 5)))
    # phase 2
    r = max(r, phase1) if spaced else phase1
    replay_at = int(rng.integers(phase1, rounds))
    while r < rounds:
        place(r, str(rng.choice(PHASE2_KINDS)), True)
        r += int(rng.integers(1, 4))

    steps, route = [], 0
    r = 0
    while r < rounds:
        for step in at.get(r, ()):
            steps.append(step)
            if rng.random() < 0.4:
                steps.append(g.observation())
        if r == replay_at:
            steps.append(dict(op="replay", route=route % 3, first=r))
            c = 1
        else:
            c = int(rng.choice([1, 1, 1, 2, 5]))
            stop = min([x for x in list(at) + [replay_at, rounds] + list(alone) + [a + 1 for a in alone] if x > r])
            c = min(c, stop - r)
            steps.append(dict(op="rounds", c=c, route=route % 3, first=r, taken=r in taken,
                              deferrals=taken.get(r, [])))
        a, b = sorted(rng.integers(0, n + 1, size=2).tolist())
        steps[-1]["digest_range"] = (a, b)
        route += 1
        r += c
        for _ in range(int(rng.integers(0, 3))):
            steps.append(g.observation())
    steps.append(dict(op="observe", what="read_full"))
    steps.append(dict(op="observe", what="pref"))
    sched = dict(seed=seed, n=n, m=m, k=k, engine_seed=engine_seed, byz=g.byz, init_mode=init_mode,
                 init_param=init_param, rounds=rounds, phase1=phase1, taken_seed=g.taken_seed, options=initial,
                 steps=steps)
    return sched, dict(at=at, kinds=kinds, replay_at=replay_at)


# ---- lossy lives: a life of the kind above with loss stretches laid over it
N_LOSSY_SEEDS = 16
LOSS_SKIP, LOSS_NEUTRAL = 0, 1
SKIP_P, NEUTRAL_P = (0.10, 0.25, 0.60), (0.05, 0.15)
THR_MAX = 2**32 - 1
DOWN_KINDS = ("none", "few", "ends", "word")  # and "all", once
LOSSY_K = {5: 12, 2: 3, 9: 5, 13: 1}  # seed -> k; every other seed k = 8
LOSSY_BYZ = (3, 7, 11)
THR_MAX_SEED, ALL_DOWN_SEED = 3, 9  # whose first stretch loses (nearly) every draw / starts with every node down
# the disturbance a stretch is laid over, by (3 * seed + stretch) mod len: every kind meets a lossy round
WANTED = ("register", "reinit", "write", "replay", "add", "options", "neutral", "kernel_flip", "register_batch",
          "replay", "set_valid", "reinit", "materialize")


def lossy_config(seed):
    """Shape, Byzantine share and k of a lossy seed."""
    n, m = SHAPES[seed % len(SHAPES)]
    return n, m, (BYZ20 if seed in LOSSY_BYZ else 0), LOSSY_K.get(seed, 8)


def make_lossy_schedule(seed):
    g = _Gen(seed, np.random.default_rng(0x105E0000 + seed), lossy_config(seed))
    sched, info = _build(g, seed, 7100 + seed)
    return _overlay(g, sched, info)


def _overlay(g, sched, info):
    """One to three loss stretches [a, b) of 2-8 rounds over the schedule: set_loss / set_responding
    steps before round a (ahead of that round's disturbances), changes part-way, the closing steps
    before round b; rounds steps cut at every such edge; taken flags cleared in [a, b + 2); regain
    rounds flagged (module docstring)."""
    rng, n, seed = g.rng, g.n, sched["seed"]
    rounds, phase1 = sched["rounds"], sched["phase1"]
    at, kinds, replay_at = info["at"], info["kinds"], info["replay_at"]
    dist = sorted(at)
    reinits = [r for r in dist if any(s["op"] == "reinit" for s in at[r])]
    first_break = min([r for r in dist if any(breaks_c_monotone(s) for s in at[r])] + [replay_at])

    def settled_end(b):
        """A stretch ending at b may be followed by a regain round: nothing disturbs b - 2 .. b + 2 (a
        re-init: b - 9 ..), and c_monotone holds through b + 2."""
        return (b + 2 < min(first_break, rounds) and not any(b - 2 <= d <= b + 2 for d in dist) and
                not any(b - 9 <= d <= b for d in reinits))

    def deferring_at(x):
        """The deferral options on in round x if plan_round can defer there (kernel 2, and virtual_votes
        or count_lazy with RecordFacts::count_bound < 120), else None."""
        cur = dict(DEFAULTS)
        cur.update({nm: v for nm, v in sched["options"] if nm in cur})
        bound, bound_r = -6, 0
        for r in dist:
            if r > x:
                break
            for step in at[r]:
                if step["op"] == "options":
                    cur.update({nm: v for nm, v in step["set"] if nm in cur})
                elif step["op"] == "reinit":
                    bound, bound_r = -6, r
                elif step["op"] in ("register", "register_batch"):
                    bound, bound_r = min(127, bound + 8 * (r - bound_r) + max_node_votes(step)), r
        lazy = cur["count_lazy"] and min(127, bound + 8 * (x - bound_r)) < 120
        if cur["kernel"] == 2 and (cur["virtual_votes"] or lazy):
            return [d for d in DEFERRALS if cur[d]]
        return None

    spans = []

    def free(a, b):
        return 1 <= a and a + 2 <= b <= rounds - 1 and all(b + 3 <= x or y + 3 <= a for x, y in spans)

    def down_set(kind):
        if kind == "few":
            return sorted(set(rng.integers(0, n, size=int(rng.integers(1, 5))).tolist()))
        if kind == "ends":
            return [0, n - 1]
        if kind == "word":  # one whole word of the responding bitset
            w = int(rng.integers(0, n // 32))
            return list(range(32 * w, 32 * w + 32))
        return list(range(n)) if kind == "all" else []

    def set_loss(thr, mode):
        return dict(op="set_loss", thr=int(thr), mode=int(mode))

    def set_responding(nodes, responds):
        return dict(op="set_responding", nodes=np.array(nodes, np.int64), responds=int(responds))

    def threshold(mode):
        return int(float(rng.choice(NEUTRAL_P if mode == LOSS_NEUTRAL else SKIP_P)) * 2**32)

    loss_steps, regain = {}, {}
    for j in range(int(rng.integers(1, 4))):
        length = int(rng.integers(2, 9))
        a = b = None
        ends = [x for x in range(12, phase1) if settled_end(x)] if g.taken_seed and j == 0 else []
        if ends:  # a phase-1 SKIP stretch that a regain round follows: late, where records finalize
            b = max(ends) if rng.random() < 0.5 else int(rng.choice(ends))
            a = max(8, b - length)
        else:
            first = (3 * seed + j) % len(WANTED)
            over = []
            for want in (WANTED[first], "materialize") + WANTED[first + 1:]:  # (materialize: the rarest)
                over = [replay_at] if want == "replay" else [r for r, kd in kinds if kd == want]
                if over:
                    break
            if over:
                d = int(rng.choice(over))
                a = max(1, d - int(rng.integers(0, length)))
                b = min(max(a + length, d + 1), rounds - 1)
        for _ in range(8):
            if a is not None and free(a, b):
                break
            a = int(rng.integers(14, rounds - 3))
            b = min(a + length, rounds - 1)
        else:
            continue
        spans.append((a, b))
        # phase 1 holds SKIP stretches only: a NEUTRAL round clears c_monotone
        mode = LOSS_SKIP if a < phase1 else int(rng.integers(0, 2))
        kind = DOWN_KINDS[(seed + j) % len(DOWN_KINDS)]
        thr = threshold(mode)
        if kind != "none" and rng.random() < 0.25:
            thr = 0  # only nodes are down
        ev = {}
        if j == 0 and seed == ALL_DOWN_SEED:  # one round with every node down, then an ordinary stretch
            down = down_set("few")
            ev[a] = [set_loss(0, mode), set_responding(down_set("all"), 0)]
            ev[a + 1] = [set_responding(down_set("all"), 1), set_loss(thr or threshold(mode), mode),
                         set_responding(down, 0)]
        else:
            if j == 0 and seed == THR_MAX_SEED:
                thr = THR_MAX
            down = down_set(kind)
            ev[a] = ([set_loss(thr, mode)] if thr or mode else []) + ([set_responding(down, 0)] if down else [])
            if b - a >= 3 and (rng.random() < 0.7 or a >= phase1):  # a change part-way
                x = int(rng.integers(a + 1, b))
                if a >= phase1 and rng.random() < 0.6:  # SKIP <-> NEUTRAL
                    mode = 1 - mode
                    thr = threshold(mode)
                    ev[x] = [set_loss(thr, mode)]
                elif down and (thr or len(down) > 1) and rng.random() < 0.5:  # a node comes back up
                    up = down.pop(int(rng.integers(0, len(down))))
                    ev[x] = [set_responding([up], 1)]
                else:  # one more goes down
                    more = int(rng.choice([i for i in range(n) if i not in down]))
                    down.append(more)
                    ev[x] = [set_responding([more], 0)]
        ev[b] = [set_loss(0, LOSS_SKIP)] + ([set_responding(sorted(down), 1)] if down else [])
        for x, steps in ev.items():
            loss_steps.setdefault(x, []).extend(steps)
        if ends:
            on = deferring_at(b + 2)
            if on is not None:
                regain[b + 2] = on

    cuts = set(loss_steps) | set(regain) | {x + 1 for x in regain}
    out, pre = [], []

    def with_observation(steps):
        if rng.random() < 0.6:
            lo, hi = sorted(rng.integers(0, n + 1, size=2).tolist())
            lo = min(lo, n - 1)
            steps = steps + [dict(op="observe", what="lost", n0=lo, n1=max(hi, lo + 1))]
        return steps

    for step in sched["steps"]:
        if step["op"] not in ("rounds", "replay"):
            pre.append(step)
            continue
        first = step["first"]
        if first in loss_steps:  # ahead of the round's disturbances
            i = next((i for i, s in enumerate(pre) if s["op"] != "observe"), len(pre))
            pre[i:i] = with_observation(loss_steps.pop(first))
        out += pre
        pre = []
        if step["op"] == "replay":
            out.append(step)
            continue
        end = first + step["c"]
        lo = first
        for hi in sorted(x for x in cuts if first < x < end) + [end]:
            piece = dict(step, c=hi - lo, first=lo)
            if any(a <= lo < b + 2 for a, b in spans):  # a lossy round defers nothing; the plain round after it checks
                piece.update(taken=False, deferrals=[])
            if lo in regain:
                piece.update(taken=True, deferrals=regain[lo], regain=True)
            out.append(piece)
            if hi < end and hi in loss_steps:
                out += with_observation(loss_steps.pop(hi))
            lo = hi
    assert not loss_steps, loss_steps
    out += pre
    return dict(sched, steps=out, lossy=True, stretches=sorted(spans), regain=sorted(regain))


PEER_REFUSED = frozenset(("register", "register_batch", "add", "write"))  # record writes a peer-push engine refuses
SHARD_COUNTS = (2, 3, 4, 8)
PEER_WORLDS = (2, 4, 8)


def restrict(sched, drop):
    """A copy of the schedule without the steps whose op is in `drop`. Observations that were drawn
    after a dropped step stay, and so do the taken flags of the rounds."""
    out = dict(sched)
    out["steps"] = [step for step in sched["steps"] if step["op"] not in drop]
    return out


def target_shards(seed, m=None):
    """The target ranges of a seed's sharded life: 2, 3, 4 or 8 shards (at most one per 32-target
    block) of whole blocks, balanced to within one block (avhip.sharding.target_shard). m: the
    targets of a life whose shape is not seed_config's (the lossy lives)."""
    m = seed_config(seed)[1] if m is None else m
    blocks = (m + 31) // 32
    g = min(SHARD_COUNTS[seed % len(SHARD_COUNTS)], blocks)
    return [(32 * (r * blocks // g), min(32 * ((r + 1) * blocks // g), m)) for r in range(g)]


def peer_world(seed):
    """The number of equal node shards of a seed's peer-group life, or None where N has no such split."""
    n = seed_config(seed)[0]
    worlds = [w for w in PEER_WORLDS if n % w == 0]
    return worlds[seed % len(worlds)] if worlds else None


def max_node_votes(step):
    """The most votes one node gets in a drop-in call (what the engine adds to count_bound)."""
    if step["op"] == "register":
        return len(step["targets"])
    sizes = np.diff(step["offsets"])
    return max(int(sizes[step["nodes"] == nd].sum()) for nd in set(step["nodes"].tolist()))


def describe(step):
    """A step in one line, without its bulk data."""
    short = {}
    for key, v in step.items():
        short[key] = f"<{v.shape}>" if isinstance(v, np.ndarray) and v.size > 8 else (v.tolist() if isinstance(v, np.ndarray) else v)
    return str(short)


def breaks_c_monotone(step):
    """Whether the engine clears RecordFacts::c_monotone on this step (round_plan.h)."""
    if step["op"] in ("replay", "write"):
        return True
    if step["op"] == "set_loss":  # a NEUTRAL lossy round shifts in consider = 0
        return step["mode"] == LOSS_NEUTRAL
    if step["op"] in ("register", "register_batch"):
        return bool(np.any(step["errs"] >= np.uint32(0x80000000)))
    return step["op"] == "options" and ("warm_skip", 0) in [tuple(x) for x in step["set"]]


def pack_updates(rows, base):
    """Oracle update rows (round, node, slot, target, status) as the engine's packed words (N < 2^24)."""
    u = np.asarray(rows, np.int64).reshape(-1, 5).astype(np.uint64)
    return (((u[:, 0] - np.uint64(base)) << np.uint64(52)) | (u[:, 1] << np.uint64(28)) | (u[:, 2] << np.uint64(24)) |
            (u[:, 3] << np.uint64(2)) | u[:, 4])


class Life:
    """One schedule replayed on the oracle and on `engines` ({name: engine}; empty: the oracle alone).
    av: the binding module (decode_updates, compact_expand, compact_header, VoteRecordNotFound)."""

    def __init__(self, sched, cabi, engines=None, av=None):
        self.s, self.cabi, self.engines, self.av = sched, cabi, dict(engines or {}), av
        self.valid = np.ones(sched["m"], bool)
        self.thr, self.mode = 0, LOSS_SKIP  # the loss state; the down set is the reference's (self.ref.down)
        self.sim = self._new_sim(0)
        self.ref = self._new_ref(None)
        self.byz = np.array([self.sim.is_byzantine(j) for j in range(sched["n"])], bool)
        self.applied = self.finalized = 0
        self.options = {name: dict() for name in self.engines}
        self.deltas = {}  # the last rounds step's alg_bytes per engine
        self.where = ""
        self.round_hook = None  # called as (round index, sim, valid) before every sim round
        self.post_init = {}  # engine name -> options set again after every av_init_records
        self.lossy_rows = []  # the update rows of every lossy round

    def _new_sim(self, first_round):
        s = self.s
        sim = self.cabi.Sim(s["n"], s["m"], s["k"], seed=s["engine_seed"], byz_threshold=s["byz"],
                            init_mode=s["init_mode"], init_param=s["init_param"])
        sim.set_round_index(first_round)
        for t in np.flatnonzero(~self.valid):
            sim.set_valid(int(t), False)
        return sim

    def _new_ref(self, old):
        """The lossy reference round over the current Sim; the down set and the counters carry over, and
        its validity is the life's own array."""
        ref = LossyRef(self.sim, self.s["engine_seed"])
        ref.valid = self.valid
        if old is not None:
            ref.down, ref.applied, ref.lost = old.down, old.applied, old.lost
        return ref

    def lossy(self):
        """The engine's lossy(): the next sim round may lose a Response."""
        return self.thr != 0 or bool(self.ref.down)

    def set_options(self, name, opts):
        for nm, v in opts:
            self.engines[name].set_option(nm, v)
            self.options[name][nm] = v

    def _same(self, got, exp, name, what):
        ok = np.array_equal(got, exp) if isinstance(exp, np.ndarray) or isinstance(got, np.ndarray) else got == exp
        assert ok, f"{self.where}: {what} of engine '{name}' differs from the oracle; options {self.options[name]}"

    # ---- rounds and their update stream
    def _stream(self, step, exp_rows):
        a, b = step["digest_range"]
        for name, e in self.engines.items():
            base = e.log_base_round()
            words = pack_updates(exp_rows, base)
            self._same(e.updates_digest(), self.cabi.update_digest(words), name, "updates_digest")
            part = words[(exp_rows[:, 1] >= a) & (exp_rows[:, 1] < b)]
            self._same(e.updates_digest(a, b), self.cabi.update_digest(part), name, f"updates_digest({a}, {b})")
            if step["route"] == 0:
                self._same(e.fetch_updates(), exp_rows, name, "fetch_updates")
            elif step["route"] == 1:
                stream = e.fetch_compact()
                got = self.av.compact_expand(stream)
                self._same(self.av.compact_header(stream)["log_base"], base, name, "compact log_base")
                self._same(got, words, name, "fetch_compact + compact_expand")
            else:
                e.discard_updates()
            self._same(e.updates_count(), 0, name, "updates_count after the fetch")

    def _rounds(self, step):
        sim = self.sim
        before = {name: e.alg_bytes() for name, e in self.engines.items()}
        if step["op"] == "replay":
            errs = self.cabi.gen_replay_errs(self.s["engine_seed"], sim.round, 0, self.s["n"], self.s["m"], self.s["k"])
            if self.round_hook:
                self.round_hook(sim.round, sim, self.valid)
            out = [sim.run_round(errs)]
            for e in self.engines.values():
                e.replay_round_errs(errs)
        else:
            out = []
            for _ in range(step["c"]):
                if self.round_hook:
                    self.round_hook(sim.round, sim, self.valid)
                if self.lossy():
                    before_applied = self.ref.applied
                    rows = self.ref.round(self.thr, self.mode)
                    out.append((rows, self.ref.applied - before_applied))
                    self.lossy_rows.append(rows)
                else:
                    out.append(sim.run_round())
            for e in self.engines.values():
                e.run_rounds(step["c"])
        exp = np.concatenate([u for u, _ in out]) if out else np.zeros((0, 5), np.int64)
        self.applied += sum(a for _, a in out)
        self.finalized += int(np.isin(exp[:, 4], (0, 3)).sum())
        self.deltas = {name: e.alg_bytes() - before[name] for name, e in self.engines.items()}
        self._stream(step, exp)

    # ---- observations
    def _observe(self, ob):
        s, sim, what = self.s, self.sim, ob["what"]
        n, m = s["n"], s["m"]
        dump = sim.dump()
        live = (dump >> np.uint32(17)) < 128
        if what == "lost":  # the draw of the round about to run, and the Responses lost so far
            lost = lost_table(s["engine_seed"], n, s["k"], sim.round, self.thr, self.ref.down)
        for name, e in self.engines.items():
            if what == "lost":
                n0, n1 = ob["n0"], ob["n1"]
                self._same(e.sample_lost(sim.round, n0, n1), lost[n0:n1].astype(np.uint8), name, "sample_lost")
                self._same(e.lost_responses(), self.ref.lost, name, "lost_responses")
            elif what == "read_full":
                self._same(e.read_records(), dump, name, "read_records")
            elif what == "read_rect":
                n0, n1, t0, t1 = ob["n0"], ob["n1"], ob["t0"], ob["t1"]
                self._same(e.read_records(n0, n1, t0, t1), dump[n0:n1, t0:t1], name, "read_records (rectangle)")
            elif what == "cells":
                for node, t in ob["cells"]:
                    w = int(dump[node, t])
                    self._same(e.is_accepted(node, t), bool(live[node, t]) and bool((w >> 16) & 1), name, "is_accepted")
                    if live[node, t]:
                        self._same(e.get_confidence(node, t), w >> 17, name, "get_confidence")
                    else:
                        try:
                            e.get_confidence(node, t)
                            found = True
                        except self.av.VoteRecordNotFound:
                            found = False
                        self._same(found, False, name, "get_confidence of an absent record")
            elif what == "invs":
                n0, n1 = ob["n0"], ob["n1"]
                offs, tg = e.get_invs_batch(n0, n1)
                got = [tg[offs[i]:offs[i + 1]].tolist() for i in range(n1 - n0)]
                exp = [np.flatnonzero(row)[:4096].tolist() for row in (live & self.valid[None, :])[n0:n1]]
                self._same(got, exp, name, "get_invs_batch")
            elif what == "pref":  # a Byzantine node's row holds its flip-flop pattern: honest rows only
                self._same(e.read_pref()[~self.byz], sim.pref()[~self.byz], name, "read_pref")
            elif what == "census":
                n0, n1, honest = ob["n0"], ob["n1"], ob["honest_only"]
                ref = census_from_words(dump[n0:n1], ~self.byz[n0:n1] if honest else None)
                got = e.census(n0, n1, honest_only=honest)
                for key in ("target_classes", "target_count_sum", "node_classes", "count_hist"):
                    self._same(got[key], ref[key].astype(got[key].dtype), name, f"census {key}")
            elif what == "live":
                rows = ~self.byz if ob["honest_only"] else np.ones(n, bool)
                self._same(e.live_records(ob["honest_only"]), int((live & self.valid[None, :])[rows].sum()), name,
                           "live_records")

    # ---- one step on every party
    def apply(self, index, step):
        s, sim, op = self.s, self.sim, step["op"]
        self.where = f"seed {s['seed']} step {index} {describe(step)}"
        E = self.engines
        if op in ("rounds", "replay"):
            self._rounds(step)
        elif op == "observe":
            self._observe(step)
        elif op == "register":
            ts, errs = step["targets"], step["errs"]
            known = (ts >= 0) & (ts < s["m"])
            exp = sim.register_votes(step["node"], ts[known], errs[known])
            for name, e in E.items():
                st = e.register_votes(step["node"], ts, errs)
                self._same([(int(t), int(x)) for t, x in zip(ts, st) if x >= 0], exp, name, "register_votes statuses")
        elif op == "register_batch":
            nodes, offs, ts, errs = step["nodes"], step["offsets"], step["targets"], step["errs"]
            got = {name: e.register_votes_batch(nodes, offs, ts, errs) for name, e in E.items()}
            for i in range(nodes.size):
                a, b = int(offs[i]), int(offs[i + 1])
                known = (ts[a:b] >= 0) & (ts[a:b] < s["m"])
                exp = sim.register_votes(int(nodes[i]), ts[a:b][known], errs[a:b][known])
                for name in E:
                    have = [(int(ts[v]), int(got[name][v])) for v in range(a, b) if got[name][v] >= 0]
                    self._same(have, exp, name, f"register_votes_batch statuses of Response {i}")
        elif op == "set_valid":
            self.valid[step["t"]] = step["valid"]
            sim.set_valid(step["t"], step["valid"])
            for e in E.values():
                e.set_valid(step["t"], step["valid"])
        elif op == "add":
            exp = [sim.add(step["node"], int(t), int(a)) for t, a in zip(step["targets"], step["accepted"])]
            for name, e in E.items():
                self._same(e.add_targets(step["node"], step["targets"], step["accepted"]).tolist(), exp, name,
                           "add_targets")
        elif op == "materialize":
            for e in E.values():
                e.materialize()
        elif op == "reinit":
            first = sim.round
            sim.close()
            self.sim = self._new_sim(first)
            self.ref = self._new_ref(self.ref)
            for name, e in E.items():
                e.discard_updates()
                e.init_records(s["init_mode"], s["init_param"])
                self.set_options(name, self.post_init.get(name, ()))
        elif op == "options":
            if "test" in E:
                self.set_options("test", step["set"])
        elif op == "set_loss":
            self.thr, self.mode = step["thr"], step["mode"]
            for e in E.values():
                e.set_loss(step["thr"], step["mode"])
        elif op == "set_responding":
            self.ref.set_responding(step["nodes"], step["responds"])
            for e in E.values():
                e.set_responding(step["nodes"], step["responds"])
        elif op == "write":
            sim.write_records(step["words"], step["n0"], step["t0"])
            for e in E.values():
                e.write_records(step["words"], n0=step["n0"], t0=step["t0"])
        else:
            raise AssertionError(op)
