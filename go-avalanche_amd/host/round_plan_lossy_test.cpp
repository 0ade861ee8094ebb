// CPU checks of rule R5 in csrc/round_plan.h (no GPU, no HIP): a sim round with lost Responses plans
// k_round_lossy with no deferred form and every write-back the facts demand, the combinations no
// kernel runs, what after_round leaves behind, and the plans once loss is off again. Exit status 0 =
// all passed (tests/test_round_plan_lossy.py).
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
  return {k, BL, 64, 64, PS, capped, 0, false, 0, false};  // (the initialiser every older test uses)
}
static PlanKnobs default_knobs() { return {2, true, 16, true, true, false, true, false, false}; }

static bool same_plan(const RoundPlan& a, const RoundPlan& b) {
  return a.unsupported == b.unsupported && a.kernel == b.kernel && a.mode == b.mode && a.k == b.k &&
         a.replay == b.replay && a.capped == b.capped && a.fresh == b.fresh && a.warm == b.warm && a.vv == b.vv &&
         a.vv_uniform == b.vv_uniform && a.klazy == b.klazy && a.kconsume == b.kconsume && a.hivirt == b.hivirt &&
         a.exact_pass == b.exact_pass && a.wb_votes == b.wb_votes && a.wb_counts == b.wb_counts &&
         a.wb_cpreset == b.wb_cpreset && a.ref_rows == b.ref_rows && a.uni_rows == b.uni_rows &&
         a.net_quiet_out == b.net_quiet_out && a.net_quiet_in == b.net_quiet_in && a.calm == b.calm &&
         a.lossy == b.lossy && a.loss_neutral == b.loss_neutral;
}

// one sim round with every target valid, the write-backs first as the engine makes them
static RoundPlan run_round(RecordFacts& f, const PlanShape& s, const PlanKnobs& o, int& cur, bool replay = false) {
  const RoundPlan p = plan_round(f, s, o, replay);
  if (p.wb_votes || p.wb_cpreset) {
    if (f.c_preset) f.c_unpreset();
    if (f.v_stale) f.votes_written_back();
  }
  if (p.wb_counts) f.counts_written_back();
  cur = cur == 2 ? 0 : cur + 1;
  f.after_round(p, true, false, cur);
  return p;
}

static void defaults() {
  const PlanShape s = shape_of(8, 32, false);
  CHECK(!s.lossy && !s.loss_neutral);  // what a shape list without them means
  RecordFacts f;
  f.init(true);
  const RoundPlan p = plan_round(f, s, default_knobs(), false);
  CHECK(!p.lossy && !p.loss_neutral && p.kernel == RoundKernel::Sweep && p.fresh);
}

// over facts, shapes and knobs: what a lossy round plans, and that the flag changes nothing else
static void derived() {
  const int ks[] = {1, 3, 8, 12, 16};
  const uint32_t bls[] = {1, 2, 32, 66};
  for (int k : ks)
    for (uint32_t BL : bls)
      for (int capped = 0; capped < 2; ++capped)
        for (int compat = 0; compat < 4; ++compat)
          for (int world = 0; world < 3; ++world)
            for (int comm = 0; comm < 2; ++comm)
              for (int kn = 0; kn < 8; ++kn)
                for (int fb = 0; fb < 64; ++fb)
                  for (int lm = 0; lm < 3; ++lm)
                    for (int replay = 0; replay < 2; ++replay) {
                      PlanShape s = shape_of(k, BL, capped != 0);
                      s.pub_mode = compat == 3 ? 0 : compat;
                      s.any_nopoll = compat == 3;
                      s.peer_world = world == 2 ? 4 : world;
                      s.has_comm = comm != 0;
                      PlanKnobs o = default_knobs();
                      o.kernel = kn & 1 ? 2 : 1;
                      o.virtual_votes = (kn & 2) != 0;
                      o.count_lazy = (kn & 4) != 0;
                      RecordFacts f;
                      f.warm_all = fb & 1;
                      f.v_stale = fb & 2;
                      f.k_pend = fb & 4;
                      f.fresh = fb & 8;
                      f.c_preset = (fb & 8) && (fb & 16);
                      f.c_monotone = !(fb & 32);
                      f.count_bound = fb & 1 ? 40 : -6;
                      const RoundPlan plain = plan_round(f, s, o, replay != 0);
                      s.lossy = lm != 0;
                      s.loss_neutral = lm == 2;
                      const RoundPlan p = plan_round(f, s, o, replay != 0);
                      if (!s.lossy || replay) {  // replay rounds ignore the setting
                        CHECK(same_plan(p, plain));
                        CHECK(!p.lossy && !p.loss_neutral);
                        continue;
                      }
                      CHECK(p.lossy && p.loss_neutral == s.loss_neutral && p.kernel == RoundKernel::Lossy);
                      CHECK(!p.warm && !p.vv && !p.vv_uniform && !p.klazy && !p.kconsume && !p.fresh && !p.calm);
                      CHECK(!p.ref_rows && !p.uni_rows && !p.net_quiet_out && !p.net_quiet_in);
                      // the deferred state is written back first, whatever it is
                      CHECK(p.wb_votes == f.v_stale && p.wb_counts == f.k_pend && p.wb_cpreset == f.c_preset);
                      CHECK(p.unsupported ==
                            (plain.unsupported || s.capped || s.pub_mode == 2 || s.peer_world > 1));
                      CHECK(p.k == s.k && !p.replay);
                      // what it leaves behind
                      RecordFacts g = f;
                      if (g.c_preset) g.c_unpreset();
                      if (p.wb_votes) g.votes_written_back();
                      if (p.wb_counts) g.counts_written_back();
                      g.after_round(p, true, false, 1);
                      CHECK(!g.warm_all && !g.nq_ok && !g.fresh && !g.c_preset && !g.v_stale && !g.k_pend);
                      CHECK(g.c_monotone == (f.c_monotone && !s.loss_neutral));
                      CHECK(g.count_bound == (f.count_bound + s.k < 127 ? f.count_bound + s.k : 127));
                      for (int b = 0; b < 3; ++b) CHECK(!g.rflag_ok[b] && !g.uni_ok[b]);
                      CHECK(!plans_c_preset(s, o));  // init under loss stores the consider planes
                    }
}

// a network's life: plain rounds that defer state, a lossy stretch, plain rounds again
static void life(bool neutral) {
  PlanShape s = shape_of(8, 32, false);
  const PlanKnobs o = default_knobs();
  RecordFacts f;
  int cur = 0;
  f.init(true, plans_c_preset(s, o));
  CHECK(f.c_preset);
  RoundPlan p = run_round(f, s, o, cur);
  CHECK(p.fresh && p.vv);
  for (int r = 1; r < 12; ++r) p = run_round(f, s, o, cur);
  CHECK(p.klazy && p.vv && f.v_stale && f.k_pend && f.warm_all && f.nq_ok);
  // loss on: the first lossy round writes both deferred forms back, the next ones find none
  s.lossy = true;
  s.loss_neutral = neutral;
  p = run_round(f, s, o, cur);
  CHECK(p.lossy && p.wb_votes && p.wb_counts && !p.wb_cpreset && !f.v_stale && !f.k_pend && !f.warm_all && !f.nq_ok);
  CHECK(f.c_monotone == !neutral);
  for (int r = 0; r < 5; ++r) {
    p = run_round(f, s, o, cur);
    CHECK(p.lossy && !p.wb_votes && !p.wb_counts && !p.wb_cpreset && !p.unsupported);
  }
  const int bound = f.count_bound;
  // loss off: the check sweep first, which makes the planes warm again if no neutral vote was seen
  s.lossy = s.loss_neutral = false;
  p = run_round(f, s, o, cur);
  CHECK(!p.lossy && p.kernel == RoundKernel::Sweep && p.mode == SweepMode::Check && !p.warm && !p.vv && !p.klazy);
  CHECK(f.count_bound == (bound + 8 < 127 ? bound + 8 : 127));
  CHECK(f.warm_all == !neutral);
  const int bound2 = f.count_bound;
  p = run_round(f, s, o, cur);
  if (neutral) {
    CHECK(p.mode == SweepMode::Check && !p.warm && !p.vv && !p.klazy);  // c_monotone is gone for good
  } else {
    CHECK(p.mode == SweepMode::Warm && p.warm && p.vv);  // as a network that never lost a Response
    CHECK(p.klazy == (bound2 < 120));  // (the bound counts the lossy rounds' k votes too)
  }
  // a lossy round right after init: the preset consider planes are stored first
  RecordFacts g;
  g.init(true, plans_c_preset(s, o));
  CHECK(g.c_preset && g.fresh);
  s.lossy = true;
  p = plan_round(g, s, o, false);
  CHECK(p.lossy && p.wb_cpreset && !p.fresh && !p.wb_votes && !p.wb_counts);
  run_round(g, s, o, cur);
  CHECK(!g.c_preset && !g.fresh && g.count_bound == 2);
}

static void unsupported() {
  const PlanKnobs o = default_knobs();
  RecordFacts f;
  f.init(true);
  PlanShape s = shape_of(8, 132, true);  // capped
  s.lossy = true;
  CHECK(plan_round(f, s, o, false).unsupported && !plan_round(f, s, o, true).unsupported);
  s = shape_of(8, 32, false);
  s.lossy = true;
  CHECK(!plan_round(f, s, o, false).unsupported);
  s.pub_mode = 1;  // IsAccepted literally: the kernel publishes it
  CHECK(!plan_round(f, s, o, false).unsupported);
  s.pub_mode = 2;  // the example responder's re-adds
  CHECK(plan_round(f, s, o, false).unsupported);
  s.pub_mode = 0;
  s.any_nopoll = true;  // non-polling nodes: honoured
  CHECK(!plan_round(f, s, o, false).unsupported);
  s.any_nopoll = false;
  s.has_comm = true;  // RCCL node shards: the exchange follows any kernel
  CHECK(!plan_round(f, s, o, false).unsupported);
  s.has_comm = false;
  s.peer_world = 2;  // peer-push
  CHECK(plan_round(f, s, o, false).unsupported);
  s.peer_world = 1;
  CHECK(!plan_round(f, s, o, false).unsupported);
}

int main() {
  defaults();
  derived();
  life(false);
  life(true);
  unsupported();
  std::printf("round_plan_lossy_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
