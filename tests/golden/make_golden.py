"""Generate tests/golden/reference_tests.json — golden vectors transcribed from
the reference's own tests (go-avalanche's avalanche_test.go).

Every expected value written here is an assertion of the reference test at the
cited line, expressed as data (inputs + expected outputs); nothing is computed
by this repo's oracle. The reference cannot be executed here (no Go toolchain),
so these transcriptions are what pins the oracle (see DESIGN.md "Oracle").

    python tests/golden/make_golden.py   # rewrites reference_tests.json
"""
import json
import os

NEG1 = 0xFFFFFFFF  # avalanche_test.go:8-11 negativeOne = uint32(-1)
SCORE = 128  # avalanche.go:10
INVALID, REJECTED, ACCEPTED, FINALIZED = 0, 1, 2, 3  # avalanche.go:42-56


def vote_record():
    """TestVoteRecord, avalanche_test.go:13-91 (bare VoteRecord, no deletion)."""
    steps = []

    def chk(vote, state, finalized, confidence, line):
        steps.append({"err": vote, "accepted": state, "finalized": finalized, "confidence": confidence,
                      "line": line})

    for _ in range(6):
        chk(0, False, False, 0, 34)
    chk(0, True, False, 0, 39)
    chk(NEG1, True, False, 1, 42)
    for i in range(2, 8):
        chk(0, True, False, i, 44)
    chk(NEG1, True, False, 7, 48)
    chk(NEG1, True, False, 7, 49)
    for _ in range(2, 8):
        chk(0, True, False, 7, 51)
    for i in range(8, SCORE):
        chk(0, True, False, i, 56)
    chk(1, True, True, SCORE, 60)
    for _ in range(5):
        chk(1, True, True, SCORE, 64)
    chk(1, False, False, 0, 70)
    chk(NEG1, False, False, 1, 73)
    for i in range(2, 8):
        chk(1, False, False, i, 75)
    chk(NEG1, False, False, 7, 79)
    chk(NEG1, False, False, 7, 80)
    for _ in range(2, 8):
        chk(1, False, False, 7, 82)
    for i in range(8, SCORE):
        chk(1, False, False, i, 87)
    chk(0, False, True, SCORE, 91)
    return {
        "name": "TestVoteRecord",
        "source": "avalanche_test.go:13-91",
        "initial_checks": [
            {"accepted_arg": True, "accepted": True, "finalized": False, "confidence": 0, "line": 22},
            {"accepted_arg": False, "accepted": False, "finalized": False, "confidence": 0, "line": 27},
        ],
        "start_accepted": False,
        "steps": steps,
    }


class Ops:
    def __init__(self):
        self.ops = []

    def is_accepted(self, h, expect, line):
        self.ops.append({"op": "is_accepted", "hash": h, "expect": expect, "line": line})

    def add(self, h, expect, line):
        self.ops.append({"op": "add", "hash": h, "expect": expect, "line": line})

    def poll_count(self, n, line):
        self.ops.append({"op": "poll_count", "expect": n, "line": line})

    def poll_contains(self, h, line):
        self.ops.append({"op": "poll_contains", "hash": h, "line": line})

    def register(self, node, votes, updates, line):
        self.ops.append({"op": "register", "node": node, "votes": votes, "expect_updates": updates,
                         "line": line})

    def confidence(self, h, expect, line):
        self.ops.append({"op": "confidence", "hash": h, "expect": expect, "line": line})

    def get_round(self, expect, line):
        self.ops.append({"op": "get_round", "expect": expect, "line": line})

    def inc_round(self, line):
        self.ops.append({"op": "inc_round", "line": line})


def block_register():
    """TestBlockRegister, avalanche_test.go:93-252. Block 65 = staticTestBlockMap
    entry (avalanche.go:114: work 99, valid, in active chain). eventLoop() calls
    only record RequestRecords (processor.go:235-243) and are omitted."""
    h = 65
    yes, no, neutral = [[0, h]], [[1, h]], [[NEG1, h]]
    o = Ops()
    o.is_accepted(h, False, 116)
    o.add(h, True, 119)
    o.poll_count(1, 120)
    o.poll_contains(h, 121)
    o.is_accepted(h, True, 124)
    for _ in range(6):
        o.register(0, yes, [], 129)
        o.is_accepted(h, True, 130)
        o.confidence(h, 0, 131)
    o.register(0, neutral, [], 137)
    o.is_accepted(h, True, 138)
    o.confidence(h, 0, 139)
    for i in range(1, 7):
        o.register(0, yes, [], 144)
        o.is_accepted(h, True, 145)
        o.confidence(h, i, 146)
    for _ in range(2):
        o.register(0, neutral, [], 153)
        o.is_accepted(h, True, 154)
        o.confidence(h, 6, 155)
    for _ in range(2, 8):
        o.register(0, yes, [], 161)
        o.is_accepted(h, True, 162)
        o.confidence(h, 6, 163)
    for i in range(7, SCORE):
        o.register(0, yes, [], 170)
        o.is_accepted(h, True, 171)
        o.confidence(h, i, 172)
    o.poll_count(1, 177)
    o.poll_contains(h, 178)
    o.register(0, yes, [[h, FINALIZED]], 182)
    o.poll_count(0, 193)
    o.add(h, True, 196)
    o.poll_count(1, 197)
    o.poll_contains(h, 198)
    for _ in range(6):
        o.register(0, no, [], 202)
        o.is_accepted(h, True, 203)
    o.register(0, no, [[h, REJECTED]], 209)
    o.is_accepted(h, False, 210)
    for _ in range(1, SCORE):
        o.register(0, no, [], 223)
        o.is_accepted(h, False, 224)
    o.poll_count(1, 229)
    o.poll_contains(h, 230)
    o.register(0, yes, [[h, INVALID]], 234)
    o.is_accepted(h, False, 235)
    o.poll_count(0, 246)
    o.add(h, True, 249)
    o.add(h, False, 250)
    o.is_accepted(h, True, 251)
    return {"name": "TestBlockRegister", "source": "avalanche_test.go:93-252",
            "targets": {str(h): {"accepted": True, "valid": True}}, "ops": o.ops}


def multi_block_register():
    """TestMultiBlockRegister, avalanche_test.go:254-363, EXCLUDING :307-313
    (asserts B before A in GetInvsForNextPoll, but the work sort is commented
    out at processor.go:163 and Go map order is random: flaky as shipped).
    :281 sets pindexB.isInActiveChain = true, so both targets start accepted."""
    a, b = 65, 66
    both = [[0, b], [0, a]]
    o = Ops()
    o.get_round(0, 268)  # round := p.GetRound() of a NewProcessor (processor.go:28-37 leaves it 0)
    o.is_accepted(a, False, 290)
    o.is_accepted(b, False, 291)
    o.add(a, True, 294)
    o.poll_count(1, 295)
    o.poll_contains(a, 296)
    o.register(0, [[0, a]], [], 298)
    o.get_round(0, 298)  # registering votes does not advance it
    o.inc_round(302)     # p.round++
    o.get_round(1, 302)
    o.add(b, True, 303)
    o.poll_count(2, 304)
    for _ in range(4):
        o.register(0, both, [], 318)
    for _ in range(SCORE):
        o.register(0, both, [], 325)
    o.register(0, both, [[a, FINALIZED]], 335)
    o.poll_count(1, 346)
    o.poll_contains(b, 347)
    o.register(0, [[0, b]], [[b, FINALIZED]], 351)
    o.poll_count(0, 362)
    o.get_round(1, 362)
    return {"name": "TestMultiBlockRegister", "source": "avalanche_test.go:254-363 (minus :307-313)",
            "targets": {str(a): {"accepted": True, "valid": True}, str(b): {"accepted": True, "valid": True}},
            "ops": o.ops}


def main():
    out = {
        "reference": "itsdevbear/go-avalanche @ 2025-01-17",
        "generator": "tests/golden/make_golden.py",
        "vote_record": vote_record(),
        "processor": [block_register(), multi_block_register()],
        "philox4x32_10_kat": [
            # Random123 kat_vectors, philox4x32 R=10: ctr[4], key[2] -> out[4]
            {"ctr": [0, 0, 0, 0], "key": [0, 0], "out": [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]},
            {"ctr": [0xFFFFFFFF] * 4, "key": [0xFFFFFFFF] * 2,
             "out": [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]},
            {"ctr": [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], "key": [0xA4093822, 0x299F31D0],
             "out": [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]},
        ],
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(out["vote_record"]["steps"]), "vote steps,",
          sum(len(p["ops"]) for p in out["processor"]), "processor ops")


if __name__ == "__main__":
    main()
