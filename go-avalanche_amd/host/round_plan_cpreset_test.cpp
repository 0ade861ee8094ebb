// CPU checks of the preset-consider-planes fact of csrc/round_plan.h (no GPU, no HIP): random walks
// over the named transitions of RecordFacts, driven the way the engine drives them (every path that
// reads or writes records other than a sim round stores the planes explicitly first: c_unpreset), and
// the plan's wb_cpreset over shapes and knobs. Exit status 0 = all passed
// (tests/test_round_plan_cpreset.py).
#include <cstdint>
#include <cstdio>

#include "../csrc/round_plan.h"

using namespace avk;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond) && ++g_failed <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

static PlanShape shape_of(int k, uint32_t BL, bool capped) {
  uint32_t PS = 1;
  while (PS < BL && PS < 32) PS *= 2;
  if (BL > 32) PS = (BL + 31) / 32 * 32;
  return {k, BL, 64, 64, PS, capped, 0, false, 0, false};
}
static PlanKnobs default_knobs() { return {2, true, 16, true, true, false, true, false, false}; }

// The engine's discipline, restated: `e` holds what av_engine holds for the plan.
struct Model {
  RecordFacts f;
  PlanShape s;
  PlanKnobs o;
  bool opt_c_preset = true;
  int cur = 0;
  long unpresets = 0;

  void invariant() const {
    CHECK(!f.c_preset || f.fresh);  // c_preset implies fresh
  }
  // materialize(e, votes, counts) of engine.cpp
  void materialize(bool votes, bool counts) {
    if (votes && f.c_preset) {
      f.c_unpreset();
      ++unpresets;
    }
    if (votes && f.v_stale) f.votes_written_back();
    if (counts && f.k_pend) f.counts_written_back();
  }
  void init(bool created) {
    const bool preset = created && opt_c_preset && plans_c_preset(s, o);
    f.init(created, preset);
    CHECK(f.c_preset == preset);
    // never for capped, compat (responder variants, non-polling nodes) or first-generation shapes
    const bool compat = s.pub_mode != 0 || s.any_nopoll;
    if (s.capped || compat || o.kernel != 2 || s.k > 8 || o.ablate_gather || !created || !opt_c_preset)
      CHECK(!f.c_preset);
  }
  void round(bool replay) {
    if (replay) f.replay_call();
    const RoundPlan p = plan_round(f, s, o, replay);
    if (p.unsupported) return;
    // the un-preset is requested exactly when the planes are preset and the round is not the fresh one
    CHECK(p.wb_cpreset == (f.c_preset && !p.fresh));
    if (replay || p.kernel != RoundKernel::Sweep || o.ablate_gather) CHECK(p.wb_cpreset == f.c_preset);
    materialize(p.wb_votes || p.wb_cpreset, false);
    materialize(false, p.wb_counts);
    CHECK(!f.c_preset || p.fresh);  // what the kernel is told (RoundParams::c_preset) only in a fresh round
    cur = cur == 2 ? 0 : cur + 1;
    f.after_round(p, true, false, cur);
    CHECK(!f.c_preset && !f.fresh);
  }
  void step(uint32_t t) {
    switch (t) {
      case 0: init(true); break;
      case 1: init(false); break;
      case 2: round(false); break;
      case 3: round(true); break;
      case 4:  // av_add_targets
        f.snapshot_written();
        materialize(true, true);
        f.add_targets();
        break;
      case 5:  // av_register_votes(_batch)
        f.snapshot_written();
        materialize(true, true);
        f.dropin_votes(1 + rnd(8), rnd(2) != 0);
        break;
      case 6:  // av_write_records
        f.snapshot_written();
        materialize(true, true);
        f.write_records();
        break;
      case 7:  // av_set_valid, av_set_polling
        f.snapshot_written();
        materialize(true, true);
        if (rnd(4) == 0) s.any_nopoll = !s.any_nopoll && !s.capped;
        break;
      case 8: materialize(true, true); break;  // av_materialize
      case 9:  // option "fresh" = 0
        f.snapshot_written();
        if (f.c_preset) materialize(true, false);
        f.option_fresh_off();
        break;
      case 10:  // plain options the plan reads, switched with records in place
        f.snapshot_written();
        switch (rnd(5)) {
          case 0: o.kernel = o.kernel == 2 ? 1 : 2; break;
          case 1: o.virtual_votes = !o.virtual_votes; break;
          case 2: o.ablate_gather = !o.ablate_gather; break;
          case 3: opt_c_preset = !opt_c_preset; break;
          case 4: o.vv_min_bl = o.vv_min_bl == 16 ? 64 : 16; break;
        }
        break;
      case 11:  // options "count_lazy" / "k_hi_virtual": counts written back, votes left
        f.snapshot_written();
        materialize(false, true);
        if (rnd(2)) o.count_lazy = !o.count_lazy; else o.k_hi_virtual = !o.k_hi_virtual;
        break;
      case 12:  // option "responder" (uncapped engines)
        f.snapshot_written();
        materialize(true, true);
        if (!s.capped) s.pub_mode = (int32_t)rnd(3);
        break;
      case 13: f.option_warm_skip_off(); break;
      case 14: break;  // reads (av_read_records, av_census): no transition, the form stays
    }
    invariant();
  }
};

static void walks() {
  const int ks[] = {1, 5, 8, 9};
  const uint32_t bls[] = {1, 4, 16, 32, 40};
  long presets = 0, fresh_kept = 0;
  for (int w = 0; w < 4000; ++w) {
    Model m;
    m.s = shape_of(ks[rnd(4)], bls[rnd(5)], rnd(4) == 0);
    m.o = default_knobs();
    m.invariant();
    for (int i = 0; i < 60; ++i) {
      // weighted towards init and rounds, so that presets are made and consumed often
      const uint32_t pick = rnd(24);
      const bool was = m.f.c_preset;
      m.step(pick < 6 ? 0u : pick < 10 ? 2u : pick - 10u + 1u);
      presets += !was && m.f.c_preset;
      fresh_kept += was && !m.f.c_preset && m.f.fresh;
    }
  }
  CHECK(presets > 1000);     // the walks do reach the preset state
  CHECK(fresh_kept > 100);   // ... and leave it with the records still fresh (av_set_valid, av_materialize)
}

static void life() {
  Model m;
  m.s = shape_of(8, 32, false);
  m.o = default_knobs();
  m.init(true);
  CHECK(m.f.c_preset && m.f.fresh);
  RoundPlan p = plan_round(m.f, m.s, m.o, false);
  CHECK(p.fresh && !p.wb_cpreset);
  m.round(false);
  CHECK(m.unpresets == 0 && !m.f.c_preset);  // the benchmark's epoch never pays the pass
  // a second init on a preset engine
  m.init(true);
  m.init(true);
  CHECK(m.f.c_preset);
  // a replay first: the plan asks for the un-preset, and the fact does not survive the round
  p = plan_round(m.f, m.s, m.o, true);
  CHECK(!p.fresh && p.wb_cpreset);
  m.round(true);
  CHECK(m.unpresets == 1 && !m.f.c_preset);
  // option c_preset = 0: today's planes
  m.opt_c_preset = false;
  m.init(true);
  CHECK(!m.f.c_preset && m.f.fresh);
  // init with no records
  m.opt_c_preset = true;
  m.init(false);
  CHECK(!m.f.c_preset && !m.f.fresh);
  // av_materialize un-presets and leaves the records fresh
  m.init(true);
  m.materialize(true, true);
  CHECK(!m.f.c_preset && m.f.fresh && m.unpresets == 2);
  p = plan_round(m.f, m.s, m.o, false);
  CHECK(p.fresh && !p.wb_cpreset);
}

static void derived() {
  const int ks[] = {1, 4, 8, 9};
  const uint32_t bls[] = {1, 8, 32, 40};
  for (int k : ks)
    for (uint32_t BL : bls)
      for (int capped = 0; capped < 2; ++capped)
        for (int compat = 0; compat < 4; ++compat)
          for (int replay = 0; replay < 2; ++replay)
            for (int kn = 0; kn < 8; ++kn)
              for (int fb = 0; fb < 4; ++fb) {
                PlanShape s = shape_of(k, BL, capped != 0);
                s.pub_mode = compat == 3 ? 0 : compat;
                s.any_nopoll = compat == 3;
                PlanKnobs o = default_knobs();
                o.kernel = kn & 1 ? 2 : 1;
                o.virtual_votes = (kn & 2) != 0;
                o.ablate_gather = (kn & 4) != 0;
                RecordFacts f;
                f.fresh = fb & 1;
                f.c_preset = (fb & 2) && f.fresh;
                const RoundPlan p = plan_round(f, s, o, replay != 0);
                CHECK(p.wb_cpreset == (f.c_preset && !p.fresh));
                const bool sweep_sim = k <= 8 && !capped && compat == 0 && o.kernel == 2 && !replay && !o.ablate_gather;
                CHECK(p.fresh == (f.fresh && sweep_sim));
                CHECK(plans_c_preset(s, o) == (k <= 8 && !capped && compat == 0 && o.kernel == 2 && !o.ablate_gather));
                RecordFacts g = f;
                if (p.wb_cpreset) g.c_unpreset();
                g.after_round(p, true, false, 1);
                CHECK(!g.c_preset && !g.fresh);
              }
}

int main() {
  life();
  derived();
  walks();
  std::printf("round_plan_cpreset_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
