// CPU checks of rule R6 in csrc/round_plan.h (no GPU, no HIP): a sim round over peer lists plans
// k_round_listed with no deferred form and every write-back the facts demand, with or without R5; the
// combinations no kernel runs; replay rounds ignore the lists; without lists the plan is the one the
// same inputs gave before the flag existed; what after_round leaves behind. Exit status 0 = all
// passed (tests/test_round_plan_listed.py).
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
         a.lossy == b.lossy && a.loss_neutral == b.loss_neutral && a.listed == b.listed;
}

static bool same_facts(const RecordFacts& a, const RecordFacts& b) {
  bool same = a.c_monotone == b.c_monotone && a.warm_all == b.warm_all && a.fresh == b.fresh &&
              a.count_bound == b.count_bound && a.c_preset == b.c_preset && a.v_stale == b.v_stale &&
              a.k_pend == b.k_pend && a.nq_ok == b.nq_ok;
  for (int i = 0; i < 3; ++i) same = same && a.rflag_ok[i] == b.rflag_ok[i] && a.uni_ok[i] == b.uni_ok[i];
  return same;
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
  CHECK(!s.listed && !s.lossy);  // what a shape list without the flag means
  RecordFacts f;
  f.init(true);
  const RoundPlan p = plan_round(f, s, default_knobs(), false);
  CHECK(!p.listed && !p.lossy && p.kernel == RoundKernel::Sweep && p.fresh);
}

// over the facts, shapes and knobs that host/round_plan_lossy_test.cpp walks, times the three loss
// settings: what a listed round plans, and that the flag changes nothing else
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
                      s.lossy = lm != 0;
                      s.loss_neutral = lm == 2;
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
                      const RoundPlan plain = plan_round(f, s, o, replay != 0);  // listed = false
                      CHECK(!plain.listed && plain.kernel != RoundKernel::Listed);
                      s.listed = true;
                      const RoundPlan p = plan_round(f, s, o, replay != 0);
                      if (replay) {  // replay rounds ignore the lists
                        CHECK(same_plan(p, plain));
                        continue;
                      }
                      CHECK(p.listed && p.kernel == RoundKernel::Listed && p.mode == SweepMode::Check);
                      // R5 rides along: lost slots by the loss mode, neutral only where a loss can occur
                      CHECK(p.lossy == s.lossy && p.loss_neutral == (s.lossy && s.loss_neutral));
                      CHECK(!p.warm && !p.vv && !p.vv_uniform && !p.klazy && !p.kconsume && !p.fresh && !p.calm);
                      CHECK(!p.ref_rows && !p.uni_rows && !p.net_quiet_out && !p.net_quiet_in);
                      // the deferred state is written back first, whatever it is
                      CHECK(p.wb_votes == f.v_stale && p.wb_counts == f.k_pend && p.wb_cpreset == f.c_preset);
                      CHECK(p.unsupported ==
                            (plain.unsupported || s.capped || s.pub_mode == 2 || s.peer_world > 1));
                      CHECK(p.k == s.k && !p.replay && p.capped == s.capped && p.hivirt == plain.hivirt &&
                            p.exact_pass == plain.exact_pass);
                      // what it leaves behind: what the lossy round of the same loss setting leaves
                      RecordFacts g = f;
                      if (g.c_preset) g.c_unpreset();
                      if (p.wb_votes) g.votes_written_back();
                      if (p.wb_counts) g.counts_written_back();
                      RecordFacts h = g;
                      g.after_round(p, true, false, 1);
                      CHECK(!g.warm_all && !g.nq_ok && !g.fresh && !g.c_preset && !g.v_stale && !g.k_pend);
                      CHECK(g.c_monotone == (f.c_monotone && !(s.lossy && s.loss_neutral)));
                      CHECK(g.count_bound == (f.count_bound + s.k < 127 ? f.count_bound + s.k : 127));
                      for (int b = 0; b < 3; ++b) CHECK(!g.rflag_ok[b] && !g.uni_ok[b]);
                      if (s.lossy) {
                        h.after_round(plain, true, false, 1);
                        CHECK(same_facts(g, h));
                      }
                      CHECK(!plans_c_preset(s, o));  // init under lists stores the consider planes
                    }
}

// The plan with listed = false, against the values the same inputs gave before the flag existed: a
// network's life round by round (the sequence host/round_plan_lossy_test.cpp pins for R5).
static void parent_plans() {
  PlanShape s = shape_of(8, 32, false);
  const PlanKnobs o = default_knobs();
  RecordFacts f;
  int cur = 0;
  f.init(true, plans_c_preset(s, o));
  CHECK(f.c_preset);
  RoundPlan p = run_round(f, s, o, cur);
  CHECK(p.kernel == RoundKernel::Sweep && p.mode == SweepMode::Fresh && p.fresh && p.vv && !p.listed && !p.lossy);
  CHECK(!p.wb_votes && !p.wb_counts && !p.wb_cpreset);
  p = run_round(f, s, o, cur);
  CHECK(p.kernel == RoundKernel::Sweep && p.mode == SweepMode::Warm && p.warm && p.vv && p.klazy && p.net_quiet_out);
  for (int r = 2; r < 12; ++r) p = run_round(f, s, o, cur);
  CHECK(p.klazy && p.vv && p.calm && p.net_quiet_in && f.v_stale && f.k_pend && f.warm_all && f.nq_ok);
  s.lossy = true;
  p = run_round(f, s, o, cur);
  CHECK(p.kernel == RoundKernel::Lossy && p.lossy && !p.listed && p.wb_votes && p.wb_counts);
}

// a network's life: plain rounds that defer state, a listed stretch, plain rounds again
static void life(bool lossy, bool neutral) {
  PlanShape s = shape_of(8, 32, false);
  const PlanKnobs o = default_knobs();
  RecordFacts f;
  int cur = 0;
  f.init(true, plans_c_preset(s, o));
  RoundPlan p = run_round(f, s, o, cur);
  CHECK(p.fresh && p.vv);
  for (int r = 1; r < 12; ++r) p = run_round(f, s, o, cur);
  CHECK(p.klazy && p.vv && f.v_stale && f.k_pend && f.warm_all && f.nq_ok);
  // lists on: the first listed round writes both deferred forms back, the next ones find none
  s.listed = true;
  s.lossy = lossy;
  s.loss_neutral = neutral;
  p = run_round(f, s, o, cur);
  CHECK(p.listed && p.wb_votes && p.wb_counts && !p.wb_cpreset && !f.v_stale && !f.k_pend && !f.warm_all && !f.nq_ok);
  CHECK(f.c_monotone == !(lossy && neutral));  // falls only when a neutral loss can occur
  for (int r = 0; r < 5; ++r) {
    p = run_round(f, s, o, cur);
    CHECK(p.listed && !p.wb_votes && !p.wb_counts && !p.wb_cpreset && !p.unsupported);
  }
  // a replay round in between runs as it always did
  RecordFacts fr = f;
  int cr = cur;
  p = run_round(fr, s, o, cr, true);
  CHECK(!p.listed && p.replay && p.mode == SweepMode::Replay && p.kernel == RoundKernel::Sweep);
  const int bound = f.count_bound;
  // lists cleared: the check sweep first, which makes the planes warm again if no neutral vote was seen
  s.listed = s.lossy = s.loss_neutral = false;
  p = run_round(f, s, o, cur);
  CHECK(!p.listed && !p.lossy && p.kernel == RoundKernel::Sweep && p.mode == SweepMode::Check && !p.warm && !p.vv &&
        !p.klazy);
  CHECK(f.count_bound == (bound + 8 < 127 ? bound + 8 : 127));
  CHECK(f.warm_all == !(lossy && neutral));
  p = run_round(f, s, o, cur);
  if (lossy && neutral)
    CHECK(p.mode == SweepMode::Check && !p.warm && !p.vv && !p.klazy);
  else
    CHECK(p.mode == SweepMode::Warm && p.warm && p.vv);  // as a network that never had lists
  // a listed round right after init: the preset consider planes are stored first
  RecordFacts g;
  g.init(true, plans_c_preset(s, o));
  CHECK(g.c_preset && g.fresh);
  s.listed = true;
  p = plan_round(g, s, o, false);
  CHECK(p.listed && p.wb_cpreset && !p.fresh && !p.wb_votes && !p.wb_counts);
  run_round(g, s, o, cur);
  CHECK(!g.c_preset && !g.fresh && g.count_bound == 2);
}

static void unsupported() {
  const PlanKnobs o = default_knobs();
  RecordFacts f;
  f.init(true);
  PlanShape s = shape_of(8, 132, true);  // capped
  s.listed = true;
  CHECK(plan_round(f, s, o, false).unsupported && !plan_round(f, s, o, true).unsupported);
  s = shape_of(8, 32, false);
  s.listed = true;
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
  s.peer_world = 2;  // peer-push: the need masks are drawn from R1
  CHECK(plan_round(f, s, o, false).unsupported);
  s.peer_world = 1;
  CHECK(!plan_round(f, s, o, false).unsupported);
}

int main() {
  defaults();
  derived();
  parent_plans();
  life(false, false);
  life(true, false);
  life(true, true);
  unsupported();
  std::printf("round_plan_listed_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
