"""Writes tests/golden/fields_cases.npz, the fixture of the external-fields tests (tests/test_host_fields.py,
tests/test_gpu_fields.py), from the CPU oracle tests/ns3d_oracle.py alone:

  el_X, el_W, el_D, el_F, el_nu,     the element cases: 4 regular + 3 sliver tets with random states, histories, forces, Re in
  el_Re, el_sigma, el_theta          [5, 200], nu_t in [0.2, 5] / Re (log-uniform), sigma in [1, 30], theta in [0, 1600]
  el_R                               the oracle's residuals of those cases with everything on, both convection readings
  step_w1, step_w2                   BDF1 then BDF2 (dt = STEP["dt"]) from the transient fixture's start on its (8, 3, 3) duct with the
                                     mixture fields of STEP set from the smooth field ``smooth_m``
  visc_*, buoy_*                     the coupled fixed points on the jittered duct of make_viscosity_golden.DUCT, scalar Dirichlet
                                     data = drivers.inner_stream_inlet_data: w, c, the oracle loop's outer count and its last
                                     contraction factor (the ratio of its last two changes)
  unc_w, unc_c                       the uncoupled pair (log ratio 0, no buoyancy) with the same kappa
  inner_visc, inner_unc              mean outlet u_x over the outlet nodes with c > 0.5, of visc_* and unc_*

    python scripts/make_fields_golden.py [--out FILE]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# The coupled cases.  Chosen so that the oracle's own loop contracts to 1e-9 well inside 30 steps (factor about 0.16 for the
# viscosity ratio, 0.02 for the buoyancy) and the coupled fields differ from the uncoupled ones by a few per cent.
COUPLED = dict(Re=10.0, kappa=0.004, rtol=1e-9, visc=dict(log_ratio=float(np.log(4.0)), buoyancy=(0.0, 0.0, 0.0)),
               buoy=dict(log_ratio=0.0, buoyancy=(0.0, -2.0, 0.0)))
STEP = dict(dt=0.05, theta_coeff=4.0, log_ratio=float(np.log(3.0)), buoyancy=(0.3, -1.0, 0.2))
OUT = os.path.join(ROOT, "tests", "golden", "fields_cases.npz")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VG = _script("make_viscosity_golden")
DUCT = VG.DUCT
random_tets = VG.random_tets


def duct_problem():
    """(mesh, flow mask, flow data, scalar mask (n,), scalar data (n,)) of the coupled cases."""
    from stabilized_navier_stokes_flow_fenicsx_amd.drivers import inner_stream_inlet_data
    m, mask, g = VG.duct_problem()
    cm, cv = inner_stream_inlet_data(m)
    return m, mask, g, cm[:, 0], cv[:, 0]


def smooth_m(points):
    """A smooth nodal mixture fraction in [0, 1] (the step case, the tests' Jacobian check)."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    return 0.5 + 0.5 * np.tanh(3.0 * (0.3 - np.sqrt(y * y + z * z))) * np.cos(0.7 * x)


def inner_outlet_mean(m, w, c):
    """Mean of u_x over the outlet nodes with c > 0.5."""
    out = m.facet_nodes(m.meta["tags"]["outlet"])
    sel = out[np.asarray(c)[out] > 0.5]
    return float(np.asarray(w).reshape(-1, 4)[sel, 0].mean())


def step_problem():
    """The (8, 3, 3) duct of the transient fixture and its start state."""
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    m = M.duct_mesh((8, 3, 3), 2.0)
    mask, g = B.duct_bcs(m).flatten()
    w0 = np.load(os.path.join(ROOT, "tests", "golden", "transient_duct_8x3x3.npz"))["w0"]
    return m, mask, g, w0, 50.0


def build():
    import ns3d_oracle as NS
    rng = np.random.default_rng(20261)
    X = np.concatenate([random_tets(rng, 4), random_tets(rng, 3, sliver=True)])
    W = rng.normal(size=(7, 16))
    Dn, Fn = rng.normal(size=(7, 4, 3)), rng.normal(size=(7, 4, 3))
    Re = rng.uniform(5.0, 200.0, size=7)
    nu = 10.0 ** rng.uniform(np.log10(0.2), np.log10(5.0), size=7) / Re
    sigma, theta = rng.uniform(1.0, 30.0, size=7), rng.uniform(0.0, 1600.0, size=7)
    el_R = np.stack([np.concatenate([NS.element(X[i][None], W[i][None], Re[i], d=Dn[i][None], f=Fn[i][None], nu_t=nu[i:i + 1], sigma=sigma[i],
                                                theta=theta[i], stress_div=True, corrected_convection=c, want_jac=False)[0] for i in range(7)])
                     for c in (False, True)])
    out = dict(el_X=X, el_W=W, el_D=Dn, el_F=Fn, el_nu=nu, el_Re=Re, el_sigma=sigma, el_theta=theta, el_R=el_R)
    # one BDF1 and one BDF2 step with both fields
    m, mask, g, w0, Re_s = step_problem()
    nu_t, f = NS.mixture_fields(m.points, m.tets, smooth_m(m.points), Re_s, STEP["log_ratio"], STEP["buoyancy"])
    w1, _ = NS.step(m.points, m.tets, mask, g, Re_s, w0, w0, STEP["dt"], 1, STEP["theta_coeff"], f=f, nu_t=nu_t)
    w2, _ = NS.step(m.points, m.tets, mask, g, Re_s, w1, w0, STEP["dt"], 2, STEP["theta_coeff"], f=f, nu_t=nu_t)
    out.update(step_w1=w1, step_w2=w2)
    # the coupled fixed points
    m, mask, g, cm, cv = duct_problem()
    C = COUPLED
    w0 = NS.stokes_start(m.points, m.tets, mask, g)
    out["duct_stokes"] = w0
    for name in ("visc", "buoy", "unc"):
        kw = C[name] if name != "unc" else dict(log_ratio=0.0, buoyancy=(0.0, 0.0, 0.0))
        w, c, ch = NS.coupled(m.points, m.tets, mask, g, C["Re"], w0, C["kappa"], cm, cv, rtol=C["rtol"], **kw)
        out[name + "_w"], out[name + "_c"] = w, c
        if name != "unc":
            out[name + "_outer"], out[name + "_factor"] = len(ch), ch[-1] / ch[-2]
    out["inner_visc"] = inner_outlet_mean(m, out["visc_w"], out["visc_c"])
    out["inner_unc"] = inner_outlet_mean(m, out["unc_w"], out["unc_c"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    out = build()
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes; outer steps visc {out['visc_outer']} (factor {out['visc_factor']:.3f}) "
          f"buoy {out['buoy_outer']} (factor {out['buoy_factor']:.3f}); inner-stream outlet mean visc {out['inner_visc']:.6f} "
          f"uncoupled {out['inner_unc']:.6f}")


if __name__ == "__main__":
    main()
