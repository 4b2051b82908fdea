"""Model-based sequence fuzz beyond the committed seeds (dev tool): python scripts/probes/sequence_fuzz.py SEED [N_PLANS]

Plans SEED .. SEED + N_PLANS - 1 of tests/sequence_plans.py, each on the config (seed mod the committed configs), applied
to tests/index_model.ModelIndex and to a real handle by tests/sequence_exec.Pair: every mutation, every search form and
every rejected op checked against the model, as tests/test_gpu_sequence.py does for the committed seeds.  A mismatch prints
the seed, the step and the op; reduce it to a scripted ordering in that file.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import vrod_amd as va                    # noqa: E402
from oracle import oracle as O           # noqa: E402
import sequence_plans as S               # noqa: E402
from sequence_exec import Pair           # noqa: E402

O.build()
va.load()
seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n_plans = int(sys.argv[2]) if len(sys.argv) > 2 else 4
bad = 0
for seed in range(seed0, seed0 + n_plans):
    cfg = S.COMMITTED[seed % len(S.COMMITTED)][1]
    t0 = time.time()
    plan = S.make_plan(seed, cfg)
    cov = S.coverage(plan, cfg)
    try:
        with Pair(va, cfg, seed) as p:
            p.run_plan(plan)
        verdict = "ok"
    except AssertionError as e:
        bad += 1
        verdict = f"MISMATCH {e}"
    print(f"seed {seed} {cfg.name}: {len(plan)} steps, growths {cov['a']}, rows {cov['final_rows']}, {time.time() - t0:.1f} s: {verdict}", flush=True)
print(f"seeds {seed0} .. {seed0 + n_plans - 1}: {bad} plan(s) with a mismatch")
sys.exit(1 if bad else 0)
