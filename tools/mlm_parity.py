"""Observed parity of the MLM step against the reference's golden values, per fixture, quantity and dtype (GPU):

  python tools/mlm_parity.py [--out profiles/mlm_parity.json]

runs the comparisons of tests/test_mlm_gpu.py::test_mlm_step_matches_reference_golden and records the errors they measure next to the
bounds the test asserts (TOL)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_mlm_gpu as T  # noqa: E402
from tests import mlm_oracle as M  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_parity.json"))
    a = ap.parse_args()
    rec = {"bounds": T.TOL, "reference": "tests/golden/mlm_*.npz (the reference's own compute_mlm / compute_itm_wpa, fp32 on the CPU)", "observed": {}}
    for name in M.FIXTURES:
        for dtype in ("f32", "bf16"):
            obs, bad, *_ = T.compare_with_golden(name, dtype)
            rec["observed"][f"{name}/{dtype}"] = {k: (float(v) if not isinstance(v, int) else v) for k, v in obs.items()}
            rec["observed"][f"{name}/{dtype}"]["outside_bounds"] = [list(b) for b in bad]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec["observed"], indent=1))
