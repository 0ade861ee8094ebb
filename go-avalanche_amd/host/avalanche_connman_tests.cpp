// avalanche_connman_tests.cpp — Engine::SetConnmans / ClearConnmans / UnsentPolls of the C++ mirror:
// batched rounds in which every node polls from its own Connman (net.go:11-31, processor.go:173-182).
// A network split into two halves that cannot see each other finalizes each half on its own value;
// with the Connmans cleared the whole network decides the next target together; a node that knows
// fewer than k peers leaves its other polls unsent. Run by tests/test_gpu_connman.py (-m gpu). Exit
// code = number of failures.
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

constexpr int kNodes = 16, kHalf = 8, kK = 4;

// how each node's record of `h` ended, from the StatusUpdates: +1 finalized accepted, -1 finalized
// rejected (Status Invalid, avalanche.go:42-56), 0 not finalized
std::vector<int> outcomes(const std::vector<uint64_t>& updates) {
  std::vector<int> out(kNodes, 0);
  for (uint64_t u : updates) {
    const int st = av_update_status(u);
    if (st == AV_STATUS_FINALIZED) out[(size_t)av_update_node(u)] = 1;
    if (st == AV_STATUS_INVALID) out[(size_t)av_update_node(u)] = -1;
  }
  return out;
}

void partition_then_whole() {
  EngineOptions o;
  o.n_nodes = kNodes;
  o.n_targets = 64;
  o.k = kK;
  auto engine = std::make_shared<Engine>(o);
  // every node's Connman holds the other nodes of its half, added in descending order and twice
  std::vector<Connman> connmans(kNodes);
  std::vector<Processor> procs;
  for (NodeID j = 0; j < kNodes; ++j) {
    const NodeID lo = j < kHalf ? 0 : kHalf;
    for (int rep = 0; rep < 2; ++rep)
      for (NodeID q = lo + kHalf - 1; q >= lo; --q)
        if (q != j) connmans[(size_t)j].AddNode(q);
    procs.emplace_back(engine, j, &connmans[(size_t)j]);
  }
  std::vector<const Connman*> view;
  for (const Connman& c : connmans) view.push_back(&c);
  EXPECT(connmans[0].NodesIDs().size() == (size_t)kHalf - 1);
  engine->SetConnmans(view);

  // the left half sees the transaction as accepted, the right half as rejected
  const Tx yes(77, true), no(77, false);
  for (NodeID j = 0; j < kNodes; ++j) EXPECT(procs[(size_t)j].AddTargetToReconcile(j < kHalf ? yes : no));
  engine->RunRounds(60);
  EXPECT(engine->UnsentPolls() == 0);  // 7 peers each, k = 4
  const std::vector<int> first = outcomes(engine->FetchUpdates());
  for (int j = 0; j < kNodes; ++j) EXPECT(first[(size_t)j] == (j < kHalf ? 1 : -1));
  for (const auto& p : procs) EXPECT(p.GetInvsForNextPoll().empty());

  // the partition heals: the next transaction, which three nodes in four accept, is decided by all
  engine->ClearConnmans();
  const Tx yes2(78, true), no2(78, false);
  for (NodeID j = 0; j < kNodes; ++j) EXPECT(procs[(size_t)j].AddTargetToReconcile(j % 4 == 3 ? no2 : yes2));
  engine->RunRounds(80);
  const std::vector<int> second = outcomes(engine->FetchUpdates());
  for (int j = 0; j < kNodes; ++j) EXPECT(second[(size_t)j] == 1);
  EXPECT(engine->UnsentPolls() == 0);
}

void few_peers_and_refusals() {
  EngineOptions o;
  o.n_nodes = kNodes;
  o.n_targets = 64;
  o.k = kK;
  auto engine = std::make_shared<Engine>(o);
  const Tx tx(5, true);
  EXPECT(engine->AddTargetToReconcileAll(tx) == kNodes);
  // node 0 knows nobody, node 1 knows two peers, everyone else the whole network
  std::vector<Connman> connmans(kNodes);
  for (NodeID j = 2; j < kNodes; ++j)
    for (NodeID q = 0; q < kNodes; ++q)
      if (q != j) connmans[(size_t)j].AddNode(q);
  connmans[1].AddNode(9);
  connmans[1].AddNode(4);
  std::vector<const Connman*> view;
  for (const Connman& c : connmans) view.push_back(&c);
  view[0] = nullptr;
  engine->SetConnmans(view);
  engine->RunRounds(3);
  EXPECT(engine->UnsentPolls() == 3 * (kK + (kK - 2)));
  EXPECT(engine->LostResponses() == 0);
  {
    Processor isolated(engine, 0), pair(engine, 1), full(engine, 2);
    EXPECT(isolated.GetConfidence(tx) == 0);  // no vote ever arrived
    EXPECT(isolated.IsAccepted(tx));
    EXPECT(pair.GetConfidence(tx) == 0);      // 6 yes votes: the window is not full yet
    EXPECT(full.GetConfidence(tx) == 3 * kK - 6);  // every yes vote from the 7th on adds 1 (vote.go:58-69)
  }
  // a Connman that holds its own node, or a node outside the network: refused, nothing changed
  Connman self;
  self.AddNode(3);
  view[3] = &self;
  int code = 0;
  try {
    engine->SetConnmans(view);
  } catch (const Error& e) {
    code = e.code;
  }
  EXPECT(code == AV_ERR_INVALID_ARG);
  Connman far;
  far.AddNode(kNodes);
  view[3] = &far;
  code = 0;
  try {
    engine->SetConnmans(view);
  } catch (const Error& e) {
    code = e.code;
  }
  EXPECT(code == AV_ERR_INVALID_ARG);
  engine->RunRounds(1);
  EXPECT(engine->UnsentPolls() == 4 * (kK + (kK - 2)));  // the lists set before still stand
}

}  // namespace

int main() {
  try {
    partition_then_whole();
    few_peers_and_refusals();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%s Connman\n", g_failures ? "FAIL" : "PASS");
  return g_failures;
}
