// CPU checks of the calm-tiles plan flag of csrc/round_plan.h (no GPU, no HIP): RoundPlan::calm over
// shapes, knobs and facts, through a network's life, and that an option write (which goes through
// RecordFacts::snapshot_written in av_set_option) clears nq_ok. Exit status 0 = all passed
// (tests/test_round_plan_calm.py).
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
  uint32_t PS = 1;
  while (PS < BL && PS < 32) PS *= 2;
  if (BL > 32) PS = (BL + 31) / 32 * 32;
  return {k, BL, 64, 64, PS, capped, 0, false, 0, false};
}
static PlanKnobs default_knobs() { return {2, true, 16, true, true, false, true, false, false}; }

// one sim round with every target valid; buffers rotate as in the engine
static RoundPlan run_round(RecordFacts& f, const PlanShape& s, const PlanKnobs& o, int& cur, bool replay = false) {
  const RoundPlan p = plan_round(f, s, o, replay);
  if (p.wb_votes) f.votes_written_back();
  if (p.wb_counts) f.counts_written_back();
  cur = cur == 2 ? 0 : cur + 1;
  f.after_round(p, true, false, cur);
  return p;
}

static void defaults_and_life() {
  const PlanShape s = shape_of(8, 32, false);
  PlanKnobs o = default_knobs();
  CHECK(o.calm_tiles);  // what a knob list without it means: on
  RecordFacts f;
  int cur = 0;
  f.init(true);
  RoundPlan p = run_round(f, s, o, cur);  // round 0: fresh, never flags
  CHECK(p.fresh && p.vv && !p.klazy && !p.calm);
  for (int r = 1; r <= 15; ++r) {  // the klazy stretch
    p = run_round(f, s, o, cur);
    CHECK(p.klazy && p.vv && !p.vv_uniform && p.calm);
  }
  p = run_round(f, s, o, cur);  // round 16: kconsume may finalize
  CHECK(p.kconsume && !p.calm);
  p = run_round(f, s, o, cur);
  CHECK(!p.klazy && !p.calm);
  // the benchmark's epoch: re-initialised
  f.init(true);
  CHECK(!run_round(f, s, o, cur).calm);
  CHECK(run_round(f, s, o, cur).calm);
  // the option off: today's plan, every other flag as it was
  PlanKnobs off = o;
  off.calm_tiles = false;
  const RoundPlan a = plan_round(f, s, o, false), b = plan_round(f, s, off, false);
  CHECK(a.calm && !b.calm);
  CHECK(a.klazy == b.klazy && a.vv == b.vv && a.vv_uniform == b.vv_uniform && a.kernel == b.kernel &&
        a.mode == b.mode && a.net_quiet_out == b.net_quiet_out && a.net_quiet_in == b.net_quiet_in &&
        a.wb_votes == b.wb_votes && a.wb_counts == b.wb_counts && a.uni_rows == b.uni_rows &&
        a.ref_rows == b.ref_rows && a.hivirt == b.hivirt && a.kconsume == b.kconsume);
  // a replayed round inside the stretch: no sim votes, no flag
  CHECK(!plan_round(f, s, o, true).calm);
}

// av_set_option("calm_tiles", v): every option write calls facts.snapshot_written first, so the round
// after it reads no network-quiet word; the plan flag follows the knob at once
static void option_write() {
  const PlanShape s = shape_of(8, 32, false);
  PlanKnobs o = default_knobs();
  RecordFacts f;
  int cur = 0;
  f.init(true);
  for (int r = 0; r < 5; ++r) run_round(f, s, o, cur);
  CHECK(f.nq_ok && plan_round(f, s, o, false).net_quiet_in);
  for (int v = 0; v < 2; ++v) {
    f.snapshot_written();  // the option write
    o.calm_tiles = v != 0;
    CHECK(!f.nq_ok);
    const RoundPlan p = plan_round(f, s, o, false);
    CHECK(!p.net_quiet_in && p.net_quiet_out && p.calm == (v != 0));
    CHECK(!f.uni_ok[0] && !f.uni_ok[1] && !f.uni_ok[2]);
    run_round(f, s, o, cur);
    CHECK(f.nq_ok);
  }
}

static void derived() {
  const int ks[] = {1, 4, 7, 8, 9};
  const uint32_t bls[] = {1, 4, 8, 15, 16, 32, 40};
  const int bounds[] = {-6, 2, 114, 119, 120, 127};
  const uint32_t minbls[] = {1, 16, 64};
  for (int k : ks)
    for (uint32_t BL : bls)
      for (int capped = 0; capped < 2; ++capped)
        for (int compat = 0; compat < 4; ++compat)
          for (int world = 0; world < 3; ++world)
            for (int replay = 0; replay < 2; ++replay)
              for (int kn = 0; kn < 64; ++kn)
                for (uint32_t minbl : minbls)
                  for (int fb = 0; fb < 8; ++fb)
                    for (int cb : bounds) {
                      PlanShape s = shape_of(k, BL, capped != 0);
                      s.pub_mode = compat == 3 ? 0 : compat;
                      s.any_nopoll = compat == 3;
                      s.peer_world = world == 2 ? 4 : world;
                      PlanKnobs o = default_knobs();
                      o.kernel = kn & 1 ? 2 : 1;
                      o.virtual_votes = (kn & 2) != 0;
                      o.count_lazy = (kn & 4) != 0;
                      o.calm_tiles = (kn & 8) != 0;
                      o.count_changed = (kn & 16) != 0;
                      o.ablate_gather = (kn & 32) != 0;
                      o.vv_min_bl = minbl;
                      RecordFacts f;
                      f.warm_all = fb & 1;
                      f.fresh = fb & 2;
                      f.c_monotone = !(fb & 4);
                      f.count_bound = cb;
                      const RoundPlan p = plan_round(f, s, o, replay != 0);
                      CHECK(p.calm == (o.calm_tiles && p.klazy && p.vv && !p.vv_uniform && s.k == 8 &&
                                       p.kernel == RoundKernel::Sweep));
                      // in the issue's words: klazy, stale votes allowed and not the uniform-only form,
                      // k = 8, sweep kernel 2, the option on; so never where any of these fails
                      if (p.calm) {
                        CHECK(s.k == 8 && o.kernel == 2 && !s.capped && !replay && s.pub_mode == 0 && !s.any_nopoll);
                        CHECK(BL >= o.vv_min_bl && o.virtual_votes && o.count_lazy && o.calm_tiles);
                        CHECK(f.count_bound < 120 && f.warm_all && f.c_monotone && !p.fresh && !p.kconsume);
                        CHECK(p.mode == SweepMode::Warm && !o.ablate_gather);
                      }
                      // the counting build and peer groups take the same candidates
                      PlanKnobs o2 = o;
                      o2.count_changed = !o.count_changed;
                      CHECK(plan_round(f, s, o2, replay != 0).calm == p.calm);
                      // the flag changes nothing else the facts record
                      PlanKnobs o3 = o;
                      o3.calm_tiles = !o.calm_tiles;
                      RecordFacts g = f, h = f;
                      g.after_round(p, true, false, 1);
                      h.after_round(plan_round(f, s, o3, replay != 0), true, false, 1);
                      CHECK(g.v_stale == h.v_stale && g.k_pend == h.k_pend && g.nq_ok == h.nq_ok &&
                            g.count_bound == h.count_bound && g.warm_all == h.warm_all && g.uni_ok[1] == h.uni_ok[1]);
                    }
}

int main() {
  defaults_and_life();
  option_write();
  derived();
  std::printf("round_plan_calm_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
