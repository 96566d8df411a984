"""The bits of the fused learners' outputs: every case of the two GPU parity lists (tests/fused_cases.py CASES) through FusedLearner /
FusedRecurrentLearner, with and without gradients, and the sha256 of every output tensor -- the loss, kl_row, the value loss, the values and
every gradient -- written to one JSON file.  Two builds of the library compute the same thing exactly when their files are equal:

    REX_LIB_PATH=<one build> python tools/learner_bits.py a.json;  REX_LIB_PATH=<another> python tools/learner_bits.py b.json;  cmp a.json b.json

(one process per build: a process loads the library once).  Every kernel sum runs in a fixed order, so a build's file does not change from run
to run."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fused_cases as fc   # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main(out_path):
    out = {}
    for network in ("forward", "recurrent"):
        for case in fc.CASES[network]:
            g, fl = fc.learner(network, fc.make_case(network, *case))
            for grad in (True, False):
                res = fc.run(g, fl, grad)
                names = {"policy_grads": fc.NAMES[network], "value_grads": fc.VALUE_NAMES}
                rec = out["%s/%s/%s" % (network, fc.case_id(network, case), "grad" if grad else "forward-only")] = {}
                for key, v in res.items():
                    if not isinstance(v, list):
                        rec[key] = digest(v)
                    elif grad:
                        rec.update({"%s.%s" % (key, n): digest(t) for n, t in zip(names[key], v)})
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("%d runs, %d tensors -> %s" % (len(out), sum(len(r) for r in out.values()), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
