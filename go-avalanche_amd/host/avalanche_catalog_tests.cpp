// avalanche_catalog_tests.cpp — the engine-owned Hash catalog through the C++ mirror:
// Engine::RegisterVotesBatch (av_register_votes_hashed: the device looks the hashes up) against
// per-Processor RegisterVotes (processor.go:61-122) on a twin engine, Engine::Retire, and a stream of
// more distinct hashes than the engine has target slots. Run by tests/test_gpu_catalog.py (-m gpu).
// Exit code = number of failures.
#include <cstdio>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "avalanche.hpp"

using namespace avalanche::gpu;

namespace {

int g_failures = 0;

#define EXPECT(cond)                                                                              \
  do {                                                                                            \
    if (!(cond)) {                                                                                \
      std::fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #cond);         \
      ++g_failures;                                                                               \
      return;                                                                                     \
    }                                                                                             \
  } while (0)

class Tx : public Target {
 public:
  Tx(Hash h, bool accepted) : h_(h), accepted_(accepted) {}
  Hash GetHash() const override { return h_; }
  std::string Type() const override { return "tx"; }
  bool IsAccepted() const override { return accepted_; }
  int64_t Score() const override { return 1; }
  bool IsValid() const override { return true; }

 private:
  Hash h_;
  bool accepted_;
};

std::shared_ptr<Engine> make_engine(int64_t nodes, int64_t targets) {
  EngineOptions o;
  o.n_nodes = nodes;
  o.n_targets = targets;
  o.k = 8;
  return std::make_shared<Engine>(o);
}

// the batch on one engine, one RegisterVotes per Response on its twin: the same StatusUpdates per
// Response, until records finalize; then Retire
void votes_batch_and_retire(bool* batch_ok) {
  const int64_t N = 10, M = 40, T = 30;
  auto eng = make_engine(N, M), twin = make_engine(N, M);
  std::vector<Processor> procs;
  for (NodeID j = 0; j < N; ++j) procs.emplace_back(twin, j);
  std::mt19937_64 rng(7);
  std::vector<std::unique_ptr<Tx>> txs;
  for (int64_t j = 0; j < T; ++j) txs.push_back(std::make_unique<Tx>((Hash)rng(), j % 2 == 0));
  txs[1] = std::make_unique<Tx>(0, false);  // hashes no sentinel could stand for
  txs[2] = std::make_unique<Tx>(-1, true);
  txs[4] = std::make_unique<Tx>(INT64_MIN, true);
  for (auto& t : txs) {
    EXPECT(eng->AddTargetToReconcileAll(*t) == N);
    EXPECT(twin->AddTargetToReconcileAll(*t) == N);
    EXPECT(eng->Find(t->GetHash()) == twin->Find(t->GetHash()) && eng->Find(t->GetHash()) >= 0);
  }
  int finalized = 0;
  for (int batch = 0; batch < 14; ++batch) {
    std::vector<NodeID> nodes;
    std::vector<Response> responses;
    for (int r = 0; r < 3 * N; ++r) {
      std::vector<Vote> votes;
      for (int rep = 0; rep < 4; ++rep)
        for (int64_t j = 0; j < T; ++j) {
          // every third target only ever hears yes (it finalizes); the others a mix with neutral votes
          const uint32_t err = j % 3 == 0 ? 0u : (uint32_t)(rng() % 4 == 0 ? (rng() % 2 ? 1u : 0x80000000u) : 0u);
          votes.push_back(NewVote(err, txs[(size_t)j]->GetHash()));
          if (rng() % 9 == 0) votes.push_back(NewVote(0, (Hash)rng()));  // a hash nobody added (:95-99)
        }
      nodes.push_back((NodeID)((r * 7) % N));  // every node three times, interleaved
      responses.push_back(NewResponse(batch, 0, std::move(votes)));
    }
    std::vector<std::vector<StatusUpdate>> got;
    eng->RegisterVotesBatch(nodes, responses, &got);
    EXPECT(got.size() == responses.size());
    for (size_t i = 0; i < responses.size(); ++i) {
      std::vector<StatusUpdate> exp;
      EXPECT(procs[(size_t)nodes[i]].RegisterVotes(0, responses[i], &exp));
      EXPECT(got[i] == exp);
      for (const auto& u : exp) finalized += u.status == Status::Finalized;
    }
  }
  EXPECT(finalized > 0);
  Processor p0(eng, 0);
  for (auto& t : txs) EXPECT(p0.IsAccepted(*t) == procs[0].IsAccepted(*t));
  *batch_ok = true;

  // Retire: a target some Processor still holds stays; one that every Processor finalized goes
  int gone = 0, kept = 0;
  for (int64_t j = 0; j < T; ++j) {
    const Tx& t = *txs[(size_t)j];
    bool held = false;
    for (NodeID n = 0; n < N; ++n) {
      Processor p(eng, n);
      try {
        (void)p.GetConfidence(t);
        held = true;
      } catch (const VoteRecordNotFound&) {
      }
    }
    const int64_t slot = eng->Find(t.GetHash());
    EXPECT(slot >= 0);
    EXPECT(eng->Retire(t) == !held);
    EXPECT((eng->Find(t.GetHash()) < 0) == !held);
    (held ? kept : gone) += 1;
  }
  EXPECT(gone > 0 && kept > 0);
  Tx never(424242, true);
  EXPECT(!eng->Retire(never));
  // the freed slots are handed out again, lowest first
  Tx a(31337, true), b(-31337, false);
  const int64_t sa = eng->Intern(a), sb = eng->Intern(b);
  EXPECT(sa >= 0 && sb > sa && sb < T);
  EXPECT(eng->HashOf(sa) == 31337 && eng->HashOf(sb) == -31337);
}

// more distinct hashes than target slots over an engine's life
void hash_stream() {
  const int64_t N = 10, M = 8;
  auto eng = make_engine(N, M);
  std::mt19937_64 rng(11);
  std::vector<std::unique_ptr<Tx>> all;
  std::set<Hash> ever;
  for (int wave = 0; wave < 5; ++wave) {
    std::set<Hash> now;
    std::vector<Tx*> txs;
    for (int64_t j = 0; j < M; ++j) {
      all.push_back(std::make_unique<Tx>((Hash)rng(), true));
      txs.push_back(all.back().get());
      EXPECT(eng->AddTargetToReconcileAll(*txs.back()) == N);
      now.insert(txs.back()->GetHash());
      ever.insert(txs.back()->GetHash());
    }
    Tx extra((Hash)rng(), true);
    EXPECT(eng->AddTargetToReconcileAll(extra) == 0 && eng->Find(extra.GetHash()) < 0);  // no free slot
    EXPECT(!eng->Retire(*txs[0]));  // every Processor holds it
    int64_t finalized = 0;
    for (int r = 0; r < 60 && finalized < N * M; ++r) {
      eng->RunRounds(1);
      for (uint64_t u : eng->FetchUpdates()) {
        EXPECT(now.count(eng->HashOf(av_update_target(u))) == 1);  // this wave's hashes, not the slots' earlier ones
        finalized += av_update_status(u) == AV_STATUS_FINALIZED;
      }
    }
    EXPECT(finalized == N * M);
    for (Tx* t : txs) {
      EXPECT(eng->Retire(*t));
      EXPECT(eng->Find(t->GetHash()) < 0);
    }
  }
  EXPECT((int64_t)ever.size() == 5 * M);
}

}  // namespace

int main() {
  bool batch_ok = false;
  int before = 0;
  try {
    votes_batch_and_retire(&batch_ok);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%s RegisterVotesBatch\n", batch_ok ? "PASS" : "FAIL");
  std::printf("%s Retire\n", g_failures ? "FAIL" : "PASS");
  before = g_failures;
  try {
    hash_stream();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%s HashStream\n", g_failures > before ? "FAIL" : "PASS");
  return g_failures;
}
