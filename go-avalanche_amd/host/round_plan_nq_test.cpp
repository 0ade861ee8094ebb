// CPU checks of the network-quiet fact of csrc/round_plan.h (no GPU, no HIP): nq_ok after each named
// transition of RecordFacts, and the two plan flags derived from it over shapes and knobs. Exit status
// 0 = all passed (tests/test_round_plan_nq.py).
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

// a network inside its klazy stretch: the fresh round and `rounds` klazy rounds behind it
static RecordFacts in_stretch(const PlanShape& s, const PlanKnobs& o, int& cur, int rounds = 4) {
  RecordFacts f;
  f.init(true);
  for (int r = 0; r <= rounds; ++r) run_round(f, s, o, cur);
  return f;
}

static void defaults_and_life() {
  const PlanShape s = shape_of(8, 32, false);
  const PlanKnobs o = default_knobs();
  CHECK(o.quiet_tiles && o.net_quiet && !o.count_changed);  // what a knob list without them means
  RecordFacts f;
  int cur = 0;
  CHECK(!f.nq_ok);
  f.init(true);
  CHECK(!f.nq_ok);
  RoundPlan p = run_round(f, s, o, cur);  // round 0: fresh, maintains nothing
  CHECK(p.fresh && !p.net_quiet_out && !p.net_quiet_in && !f.nq_ok);
  p = run_round(f, s, o, cur);  // round 1: the first klazy round maintains the word and reads none
  CHECK(p.klazy && p.net_quiet_out && !p.net_quiet_in && f.nq_ok);
  for (int r = 2; r <= 15; ++r) {
    p = run_round(f, s, o, cur);
    CHECK(p.klazy && p.net_quiet_out && p.net_quiet_in && f.nq_ok);
  }
  p = run_round(f, s, o, cur);  // round 16: kconsume
  CHECK(p.kconsume && !p.klazy && !p.net_quiet_out && !p.net_quiet_in && !f.nq_ok);
  p = run_round(f, s, o, cur);  // round 17 and later: counts may reach 120
  CHECK(!p.klazy && !p.net_quiet_out && !p.net_quiet_in && !f.nq_ok);
  // the benchmark's epoch: re-initialised, the next stretch starts from nothing
  f.init(true);
  CHECK(!f.nq_ok);
  run_round(f, s, o, cur);
  CHECK(!f.nq_ok);
  p = run_round(f, s, o, cur);
  CHECK(p.net_quiet_out && !p.net_quiet_in && f.nq_ok);
}

static void transitions() {
  const PlanShape s = shape_of(8, 32, false);
  const PlanKnobs o = default_knobs();
  int cur = 0;
  // every named transition clears the fact, and the plan then passes no input word
  for (int t = 0; t < 12; ++t) {
    RecordFacts f = in_stretch(s, o, cur);
    CHECK(f.nq_ok && plan_round(f, s, o, false).net_quiet_in);
    switch (t) {
      case 0: f.snapshot_written(); break;  // av_set_valid, av_set_option, av_set_polling, exchange set-up
      case 1: f.init(true); break;
      case 2: f.init(false); break;
      case 3: f.add_targets(); break;
      case 4: f.dropin_votes(1, false); break;
      case 5: f.dropin_votes(1, true); break;
      case 6: f.write_records(); break;
      case 7: f.replay_call(); break;
      case 8: f.votes_written_back(); break;   // every write-back, av_materialize included
      case 9: f.counts_written_back(); break;
      case 10: f.responder_readds(); break;
      case 11: f.after_round(plan_round(f, s, o, true), true, false, cur); break;  // a replay round
    }
    CHECK(!f.nq_ok);
    const RoundPlan p = plan_round(f, s, o, false);
    CHECK(!p.net_quiet_in);
    CHECK(!p.klazy || p.net_quiet_out);  // a klazy round starts the word again
  }
  // the two option transitions go through av_set_option's snapshot_written; alone they touch facts
  // that end the klazy rounds (warm_skip) or none the path depends on (fresh)
  RecordFacts f = in_stretch(s, o, cur);
  f.option_warm_skip_off();
  CHECK(!plan_round(f, s, o, false).klazy && !plan_round(f, s, o, false).net_quiet_out);
  // whatever clears uni_ok clears nq_ok
  f = in_stretch(s, o, cur);
  CHECK(f.uni_ok[cur] && f.nq_ok);
  f.snapshot_written();
  for (int b = 0; b < 3; ++b) CHECK(!f.uni_ok[b]);
  CHECK(!f.nq_ok);
  // a write-back, then rounds: the round after it maintains the word again and reads none
  f = in_stretch(s, o, cur);
  f.votes_written_back();
  f.counts_written_back();
  RoundPlan p = run_round(f, s, o, cur);
  CHECK(p.klazy && p.net_quiet_out && !p.net_quiet_in && f.nq_ok);
  p = run_round(f, s, o, cur);
  CHECK(p.net_quiet_in);
  // reads change nothing: no transition exists for them (av_read_records, av_read_pref, av_census)
}

static void derived() {
  const int ks[] = {1, 4, 7, 8, 9};
  const uint32_t bls[] = {1, 4, 8, 32, 40};
  const int bounds[] = {-6, 2, 114, 119, 120, 127};
  for (int k : ks)
    for (uint32_t BL : bls)
      for (int capped = 0; capped < 2; ++capped)
        for (int compat = 0; compat < 4; ++compat)
          for (int world = 0; world < 3; ++world)
            for (int comm = 0; comm < 2; ++comm)
              for (int replay = 0; replay < 2; ++replay)
                for (int kn = 0; kn < 128; ++kn)
                  for (int fb = 0; fb < 8; ++fb)
                    for (int cb : bounds) {
                      PlanShape s = shape_of(k, BL, capped != 0);
                      s.pub_mode = compat == 3 ? 0 : compat;
                      s.any_nopoll = compat == 3;
                      s.peer_world = world == 2 ? 4 : world;
                      s.has_comm = comm != 0;
                      PlanKnobs o = default_knobs();
                      o.kernel = kn & 1 ? 2 : 1;
                      o.virtual_votes = (kn & 2) != 0;
                      o.count_lazy = (kn & 4) != 0;
                      o.uni_rows = (kn & 8) != 0;
                      o.quiet_tiles = (kn & 16) != 0;
                      o.net_quiet = (kn & 32) != 0;
                      o.count_changed = (kn & 64) != 0;
                      RecordFacts f;
                      f.warm_all = fb & 1;
                      f.nq_ok = fb & 2;
                      f.k_pend = fb & 4;
                      f.count_bound = cb;
                      const RoundPlan p = plan_round(f, s, o, replay != 0);
                      const bool single = s.peer_world <= 1 && !s.has_comm && !o.count_changed;
                      CHECK(p.net_quiet_out == (p.klazy && p.kernel == RoundKernel::Sweep && single && o.quiet_tiles &&
                                                o.net_quiet));
                      CHECK(p.net_quiet_in == (p.net_quiet_out && f.nq_ok));
                      // never with k < 8, kernel 1, capped or first-generation shapes, replay, kconsume
                      CHECK(!p.net_quiet_out || (s.k == 8 && o.kernel == 2 && !s.capped && !replay && !p.kconsume &&
                                                 s.pub_mode == 0 && !s.any_nopoll && f.count_bound < 120));
                      RecordFacts g = f;
                      g.after_round(p, true, false, 1);
                      CHECK(g.nq_ok == p.net_quiet_out);
                    }
}

int main() {
  defaults_and_life();
  transitions();
  derived();
  std::printf("round_plan_nq_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
