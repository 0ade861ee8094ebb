// CPU checks of csrc/round_plan.h (no GPU, no HIP): the invariants of plan_round over the full cross
// product of its inputs, the fact sequences of the usual runs, and the sweep grid's arithmetic
// against the two formulas it replaced. Exit status 0 = all passed (tests/test_round_plan.py).
#include <cstdio>

#include "../csrc/round_plan.h"

using namespace avk;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond) && ++g_failed <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
  } while (0)

static PlanShape shape_of(int k, uint32_t BL, bool capped) {
  uint32_t PS = 1;  // avk::pref_stride: a power of two up to 32 words, then multiples of 32
  while (PS < BL && PS < 32) PS *= 2;
  if (BL > 32) PS = (BL + 31) / 32 * 32;
  return {k, BL, 64, 64, PS, capped, 0, false, 0, false};
}
static PlanKnobs default_knobs() { return {2, true, 16, true, true, false, true, false, false}; }

// what launch_sweep_k's chain picked from RoundParams before the plan carried the mode
static SweepMode old_chain(bool replay, bool ablate_gather, bool p_fresh, bool warm_skip, bool warm_all) {
  if (replay) return SweepMode::Replay;
  if (ablate_gather) return SweepMode::Ablate;
  if (p_fresh) return SweepMode::Fresh;
  return warm_skip && warm_all ? SweepMode::Warm : SweepMode::Check;
}

static void check_plan(const RecordFacts& f, const PlanShape& s, const PlanKnobs& o, bool replay) {
  const RoundPlan p = plan_round(f, s, o, replay);
  const bool sweep = p.kernel == RoundKernel::Sweep;
  CHECK(!p.klazy || (p.warm && s.k == 8 && f.count_bound < 120));
  CHECK(!p.kconsume || (!p.klazy && p.warm && f.k_pend));
  CHECK(!p.warm || (sweep && !replay && f.c_monotone && f.warm_all && !p.fresh && !o.ablate_gather));
  CHECK(!p.fresh || (sweep && !replay));
  CHECK(!p.vv || (s.k == 8 && (p.warm || p.fresh)));
  CHECK(!p.vv_uniform || (p.vv && s.BL < o.vv_min_bl));
  // "written back first": whenever something is deferred (the write-back of nothing is no launch)
  CHECK(p.vv || p.wb_votes == f.v_stale);
  CHECK(p.klazy || p.kconsume || p.wb_counts == f.k_pend);
  CHECK(!p.vv || !p.wb_votes);
  CHECK(!(p.klazy || p.kconsume) || !p.wb_counts);
  CHECK(sweep || !(p.vv || p.klazy || p.kconsume || p.fresh || p.warm || p.ref_rows || p.uni_rows));
  // RoundParams as round_params fills it: fresh = the plan's, warm_skip = c_monotone, warm_all
  CHECK(p.mode == old_chain(replay, o.ablate_gather, p.fresh, f.c_monotone, f.warm_all));
  CHECK(!sweep || (p.mode == SweepMode::Warm) == p.warm);
  CHECK(p.exact_pass == (f.count_bound >= 120));
  CHECK(p.hivirt == (o.k_hi_virtual && s.k == 8));
  const bool second_gen = o.kernel == 2 && s.k <= 8 && s.pub_mode == 0 && !s.any_nopoll;
  CHECK(sweep == (second_gen && !s.capped));
  CHECK((p.kernel == RoundKernel::Node) == (second_gen && s.capped));
  CHECK(p.unsupported == (s.capped && (s.pub_mode == 2 || s.any_nopoll)));
  CHECK(p.k == s.k && p.replay == replay && p.capped == s.capped);
}

static void invariants() {
  const int ks[] = {1, 4, 8, 9};
  const uint32_t bls[] = {1, 7, 8, 16, 32, 40};
  const int bounds[] = {-6, 2, 114, 119, 120, 127};
  for (int k : ks)
    for (uint32_t BL : bls)
      for (int capped = 0; capped < 2; ++capped)
        // the shapes that force the first-generation kernels: responder 1, responder 2, a non-polling
        // node; these with every knob off and every knob on, the plain shape with every combination
        for (int compat = 0; compat < 4; ++compat)
          for (int replay = 0; replay < 2; ++replay)
            for (int kn = 0; kn < 512; kn += compat ? 511 : 1) {
              PlanShape s = shape_of(k, BL, capped != 0);
              s.pub_mode = compat == 3 ? 0 : compat;
              s.any_nopoll = compat == 3;
              const PlanKnobs o{kn & 1 ? 2 : 1, (kn & 2) != 0,  kn & 4 ? 16u : 1u, (kn & 8) != 0,  (kn & 16) != 0,
                                (kn & 32) != 0, (kn & 64) != 0, (kn & 128) != 0,   (kn & 256) != 0};
              for (int fb = 0; fb < 32; ++fb)
                for (int cb : bounds) {
                  RecordFacts f;
                  f.c_monotone = fb & 1;
                  f.warm_all = fb & 2;
                  f.fresh = fb & 4;
                  f.v_stale = fb & 8;
                  f.k_pend = fb & 16;
                  f.count_bound = cb;
                  check_plan(f, s, o, replay != 0);
                }
            }
}

// one sim round with every target valid; buffers rotate as in the engine
static RoundPlan run_round(RecordFacts& f, const PlanShape& s, const PlanKnobs& o, int& cur) {
  const RoundPlan p = plan_round(f, s, o, false);
  if (p.wb_votes) f.votes_written_back();
  if (p.wb_counts) f.counts_written_back();
  cur = cur == 2 ? 0 : cur + 1;
  f.after_round(p, true, false, cur);
  return p;
}

static void sequences() {
  const PlanShape s = shape_of(8, 32, false);
  PlanKnobs o = default_knobs();
  RecordFacts f;
  int cur = 0;
  CHECK(f.count_bound == 127 && f.c_monotone && !f.warm_all && !f.fresh);
  f.init(true);
  CHECK(f.count_bound == -6 && f.fresh && !f.warm_all && !f.v_stale && !f.k_pend);
  RoundPlan p = run_round(f, s, o, cur);  // round 0
  CHECK(p.kernel == RoundKernel::Sweep && p.mode == SweepMode::Fresh);
  CHECK(p.fresh && p.vv && p.hivirt && !p.klazy && !p.kconsume && !p.warm && !p.wb_votes && !p.wb_counts);
  CHECK(f.count_bound == 2 && f.k_pend && f.warm_all && f.v_stale && !f.fresh);
  CHECK(f.uni_ok[1] && !f.uni_ok[0] && !f.rflag_ok[1]);
  for (int r = 1; r <= 15; ++r) {
    CHECK(f.count_bound == 2 + 8 * (r - 1));
    p = run_round(f, s, o, cur);
    CHECK(p.warm && p.vv && p.klazy && !p.kconsume && !p.fresh && !p.wb_votes && !p.wb_counts);
    CHECK(p.mode == SweepMode::Warm && !p.vv_uniform && !p.exact_pass);
  }
  CHECK(f.count_bound == 122 && f.k_pend);
  p = run_round(f, s, o, cur);  // round 16
  CHECK(p.warm && p.vv && !p.klazy && p.kconsume && !p.wb_counts && !f.k_pend);
  p = run_round(f, s, o, cur);  // round 17
  CHECK(p.warm && p.vv && !p.klazy && !p.kconsume && !p.wb_votes && !p.wb_counts);
  CHECK(f.count_bound == 127 && !f.k_pend && f.v_stale);

  // count_lazy = 0: the round after the fresh one applies the kHiVirt flags itself
  o.count_lazy = false;
  f.init(true);
  run_round(f, s, o, cur);
  p = run_round(f, s, o, cur);
  CHECK(p.warm && !p.klazy && p.kconsume && !f.k_pend);
  o = default_knobs();

  // whatever can write a 0 consider bit ends the warm rounds, and the deferred state is written back
  for (int cause = 0; cause < 3; ++cause) {
    f = RecordFacts();
    f.init(true);
    run_round(f, s, o, cur);
    run_round(f, s, o, cur);
    CHECK(plan_round(f, s, o, false).warm);
    f.dropin_votes(3, false);  // considered votes: still warm, the bound follows
    CHECK(plan_round(f, s, o, false).warm && f.count_bound == 13);
    if (cause == 0) f.dropin_votes(1, true);
    if (cause == 1) f.write_records();
    if (cause == 2) f.replay_call();
    p = plan_round(f, s, o, false);
    CHECK(!p.warm && !p.vv && !p.klazy && !p.kconsume && p.mode == SweepMode::Check && p.wb_votes && p.wb_counts);
    CHECK(cause != 1 || f.count_bound == 127);
    p = plan_round(f, s, o, true);
    CHECK(p.mode == SweepMode::Replay && !p.warm && !p.vv);
  }
  f = RecordFacts();
  f.init(true);
  f.add_targets();
  CHECK(!f.fresh && !f.warm_all && f.count_bound == -6);
  run_round(f, s, o, cur);
  CHECK(f.warm_all);
  f.add_targets();
  CHECK(!f.warm_all && !plan_round(f, s, o, false).warm);
  f.init(false);  // av_create's empty planes: not fresh
  CHECK(!f.fresh && f.count_bound == -6);
  // a replay round, a round with an invalid target and the responders' re-adds leave no warm state
  f = RecordFacts();
  f.init(true);
  p = plan_round(f, s, o, false);
  f.after_round(p, /*all_valid=*/false, false, 1);
  CHECK(!f.warm_all);
  f.after_round(plan_round(f, s, o, false), true, true, 2);
  CHECK(f.warm_all && !f.rflag_ok[2]);  // ref_rows off: flags the launch reports are not trusted
  f.after_round(plan_round(f, s, o, true), true, false, 0);
  CHECK(!f.warm_all && !f.uni_ok[0]);
  f.responder_readds();
  CHECK(f.count_bound == 127 && !f.warm_all);
  f.uni_ok[1] = f.rflag_ok[2] = true;
  f.snapshot_written();
  for (int b = 0; b < 3; ++b) CHECK(!f.uni_ok[b] && !f.rflag_ok[b]);
  f.fresh = true;
  f.option_fresh_off();
  f.option_warm_skip_off();
  CHECK(!f.fresh && !f.c_monotone);
}

static void grids() {
  const uint32_t tiles_of[] = {1, 3, 4, 5, 63, 64, 1537, 98304, 500000};
  const uint32_t blocks_of[] = {0, 1, 7, 1024, 31250, 1u << 20};
  for (uint32_t tiles : tiles_of)
    for (uint32_t blocks : blocks_of) {
      // launch_sweep_k as it was
      const uint32_t need = (tiles + 3u) / 4u;
      const uint32_t grid = std::max(1u, blocks ? std::min(blocks, need) : need);
      const uint32_t waves = grid * 4u, run = (tiles + waves - 1u) / waves;
      uint64_t owners = 0;  // waves whose run [w run, w run + run) holds a tile
      for (uint32_t w = 0; w < waves; ++w) owners += (uint64_t)w * run < tiles;
      // log_writer_waves as it was
      uint64_t old_writers = tiles;
      if (blocks) {
        const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(blocks, ((uint64_t)tiles + 3) / 4));
        const uint64_t r = (tiles + g * 4 - 1) / (g * 4);
        old_writers = std::max<uint64_t>(1, (tiles + r - 1) / r);
      }
      const SweepGrid g = sweep_grid(tiles, blocks);
      CHECK(g.grid == grid && g.run == run);
      CHECK(sweep_run_waves(tiles, blocks) == owners);
      CHECK(sweep_run_waves(tiles, blocks) == old_writers);
    }
}

int main() {
  invariants();
  sequences();
  grids();
  std::printf("round_plan_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
