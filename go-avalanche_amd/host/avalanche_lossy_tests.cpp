// avalanche_lossy_tests.cpp — Engine::SetLoss / SetResponding of the C++ mirror: batched rounds in
// which Responses do not arrive (the RegisterVotes call that never happens, processor.go:66-76) or
// arrive with neutral votes (vote.go:55-56), restated on a small network whose outcome is known
// without a draw: every peer down, then up again. Run by tests/test_gpu_lossy.py (-m gpu). Exit code
// = number of failures.
#include <cstdio>
#include <memory>
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
  explicit Tx(Hash h) : h_(h) {}
  Hash GetHash() const override { return h_; }
  std::string Type() const override { return "tx"; }
  bool IsAccepted() const override { return true; }
  int64_t Score() const override { return 1; }
  bool IsValid() const override { return true; }

 private:
  Hash h_;
};

constexpr int kNodes = 6, kK = 4;

std::shared_ptr<Engine> network(std::vector<Processor>* procs, const Tx& tx) {
  EngineOptions o;
  o.n_nodes = kNodes;
  o.n_targets = 64;
  o.k = kK;
  auto engine = std::make_shared<Engine>(o);
  for (NodeID j = 0; j < kNodes; ++j) procs->emplace_back(engine, j);
  engine->AddTargetToReconcileAll(tx);
  return engine;
}

void skip_mode() {
  std::vector<Processor> procs;
  Tx tx(77);
  auto engine = network(&procs, tx);
  std::vector<NodeID> all;
  for (NodeID j = 0; j < kNodes; ++j) all.push_back(j);
  // a perfect network: every vote is a yes, 4 per round, so two rounds fill the window with no
  // conclusive vote yet (7 considered yes votes are needed, vote.go:58) and the next adds confidence
  engine->RunRounds(2);
  for (const auto& p : procs) EXPECT(p.GetConfidence(tx) == 2);
  EXPECT(engine->LostResponses() == 0);
  // every peer down: the Responses never arrive, nothing moves, whatever the number of rounds
  engine->SetResponding(all, false);
  engine->RunRounds(5);
  EXPECT(engine->Round() == 7);
  EXPECT(engine->LostResponses() == 5 * kNodes * kK);
  for (const auto& p : procs) {
    EXPECT(p.GetConfidence(tx) == 2);
    EXPECT(p.IsAccepted(tx));
  }
  EXPECT(engine->FetchUpdates().empty());  // agreeing votes append no StatusUpdate (vote.go:66-69)
  // up again: the network goes on to finalization as if the five rounds had not been
  engine->SetResponding(all, true);
  engine->RunRounds(40);
  EXPECT(engine->LostResponses() == 5 * kNodes * kK);
  for (const auto& p : procs)
    EXPECT(p.GetInvsForNextPoll().empty());  // finalized and deleted (processor.go:114-116)
  size_t finalized = 0;
  for (uint64_t u : engine->FetchUpdates()) finalized += av_update_status(u) == AV_STATUS_FINALIZED;
  EXPECT(finalized == (size_t)kNodes);
}

void neutral_mode() {
  std::vector<Processor> procs;
  Tx tx(78);
  auto engine = network(&procs, tx);
  engine->RunRounds(3);  // 12 yes votes: confidence 6
  for (const auto& p : procs) EXPECT(p.GetConfidence(tx) == 6);
  // one node down, neutral Responses: a node that draws it shifts in an unconsidered vote, which
  // neither adds confidence nor resets it while seven considered yes votes surround it
  engine->SetLoss(0, true);
  engine->SetResponding({3}, false);
  engine->RunRounds(1);
  const int64_t lost = engine->LostResponses();
  EXPECT(lost > 0 && lost <= kNodes * kK);
  for (const auto& p : procs) {
    EXPECT(p.IsAccepted(tx));
    EXPECT(p.GetConfidence(tx) >= 6 && p.GetConfidence(tx) <= 10);
  }
  // every Response neutral: the windows empty out and confidence stands still
  engine->SetLoss(0xFFFFFFFFu, true);
  engine->RunRounds(2);
  std::vector<uint16_t> conf;
  for (const auto& p : procs) conf.push_back(p.GetConfidence(tx));
  engine->RunRounds(3);
  for (size_t j = 0; j < procs.size(); ++j) EXPECT(procs[j].GetConfidence(tx) == conf[j]);
  EXPECT(engine->LostResponses() >= lost + 5 * kNodes * kK - 5 * kNodes);  // (all but ~2^-32 of them)
}

}  // namespace

int main() {
  try {
    skip_mode();
    neutral_mode();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%s Lossy\n", g_failures ? "FAIL" : "PASS");
  return g_failures;
}
