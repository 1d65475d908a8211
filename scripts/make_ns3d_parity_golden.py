"""Writes tests/golden/ns3d_parity.npz: what the three per-feature oracles that tests/ns3d_oracle.py replaced returned on the
inputs of tests/test_host_fields.py::test_without_fields_it_is_the_transient_oracle and
::test_uniform_stress_divergence_form_is_the_law_at_n_one (seeds 72 and 73, 6 tets, both convection readings):

  transient_c{0,1}_s{0,1,2}          transient_residual with the history D at the three (sigma, theta) of SIGMA_THETA
  transient_force_c{0,1}_s{0,1,2}    the same with the history D - F
  law_c{0,1}                         law_residual at n = 1 (lambda = 2.5, r = 0.05)

The old modules (tests/transient_oracle.py, tests/viscosity_oracle.py, tests/fields_oracle.py) are no longer in the tree: they
are read from the git objects of the last commit that had them, into a temporary directory.

    python scripts/make_ns3d_parity_golden.py [--rev COMMIT] [--out FILE]
"""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "ns3d_parity.npz")
REV = "35f94eb0f12ccb77e4c9fc307889e1ced08f8bba"          # the last commit with the three modules
OLD = ("transient_oracle", "viscosity_oracle", "fields_oracle")
SIGMA_THETA = ((0.0, 0.0), (7.0, 0.0), (20.0, 1600.0))
RE = 37.0


def random_tets(rng, n):
    return rng.normal(size=(n, 4, 3))                       # make_viscosity_golden.random_tets without slivers


def old_modules(rev, into):
    """The three modules of ``rev``, written into the directory ``into`` and imported from there."""
    mods = {}
    for name in OLD:
        path = os.path.join(into, name + ".py")
        with open(path, "wb") as fh:
            fh.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:tests/{name}.py"], check=True, capture_output=True).stdout)
    sys.path.insert(0, into)
    try:
        for name in OLD:
            spec = importlib.util.spec_from_file_location(name, os.path.join(into, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(into)
    return mods


def build(rev=REV):
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        mods = old_modules(rev, tmp)
    TO, VO = mods["transient_oracle"], mods["viscosity_oracle"]
    out = {}
    for c in (0, 1):
        rng = np.random.default_rng(72)                     # the draws of the first test, in its order
        X = random_tets(rng, 6)
        W, D = rng.normal(size=(6, 16)), rng.normal(size=(6, 4, 3))
        for k, (sigma, theta) in enumerate(SIGMA_THETA):
            out[f"transient_c{c}_s{k}"] = TO.transient_residual(X, torch.as_tensor(W), D, RE, sigma, theta, corrected_convection=bool(c)).numpy()
            F = rng.normal(size=(6, 4, 3))
            out[f"transient_force_c{c}_s{k}"] = TO.transient_residual(X, torch.as_tensor(W), D - F, RE, sigma, theta,
                                                                      corrected_convection=bool(c)).numpy()
        rng = np.random.default_rng(73)                     # ... and of the second
        X = random_tets(rng, 6)
        W = rng.normal(size=(6, 16))
        out[f"law_c{c}"] = VO.law_residual(X, torch.as_tensor(W), RE, 2.5, 1.0, 0.05, corrected_convection=bool(c)).numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default=REV)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    np.savez_compressed(args.out, **build(args.rev))
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
