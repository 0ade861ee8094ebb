// avalanche_admit_tests.cpp — Engine::AddTargetToReconcileAll (every Processor of the engine adds a
// Target when it appears, main.go:97-103) against the per-Processor AddTargetToReconcile
// (processor.go:45-58) on the C++ mirror. Run by tests/test_gpu_admit.py (-m gpu). Exit code =
// number of failures.
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
  Tx(Hash h, bool valid, bool accepted) : h_(h), valid_(valid), accepted_(accepted) {}
  Hash GetHash() const override { return h_; }
  std::string Type() const override { return "tx"; }
  bool IsAccepted() const override { return accepted_; }
  int64_t Score() const override { return 1; }
  bool IsValid() const override { return valid_; }

 private:
  Hash h_;
  bool valid_, accepted_;
};

void admit_all() {
  EngineOptions o;
  o.n_nodes = 5;
  o.n_targets = 64;
  o.k = 1;
  auto engine = std::make_shared<Engine>(o);
  std::vector<Processor> procs;
  for (NodeID j = 0; j < 5; ++j) procs.emplace_back(engine, j);
  Tx yes(65, true, true), no(66, true, false), invalid(67, false, true);

  EXPECT(engine->AddTargetToReconcileAll(yes) == 5);
  for (const auto& p : procs) {
    EXPECT(p.IsAccepted(yes));
    EXPECT(p.GetInvsForNextPoll().size() == 1);
  }
  EXPECT(engine->AddTargetToReconcileAll(yes) == 0);  // every Processor holds it (:50-53)
  EXPECT(!procs[2].AddTargetToReconcile(yes));
  EXPECT(engine->AddTargetToReconcileAll(invalid) == 0);  // !IsValid (:46-48)
  EXPECT(engine->Find(67) < 0);

  EXPECT(procs[3].AddTargetToReconcile(no));  // one Processor saw it first
  EXPECT(engine->AddTargetToReconcileAll(no) == 4);
  for (const auto& p : procs) {
    EXPECT(!p.IsAccepted(no));
    EXPECT(p.GetInvsForNextPoll().size() == 2);
  }
}

}  // namespace

int main() {
  try {
    admit_all();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%s AdmitAll\n", g_failures ? "FAIL" : "PASS");
  return g_failures;
}
