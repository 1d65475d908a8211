"""The least-squares problem of the two FGMRES loops (csrc/sns_policy.h: policy::GivensLsq<T>, T = double for fgmres of
csrc/sns_krylov.hip and std::complex<double> for cfgmres of csrc/sns_shifted.hip): tests/givens_lsq_main.cpp, its own executable
built with AddressSanitizer + UBSan and run directly, scripted columns in, numbers out.

1. Against a transcription of the two loops as they stood before the class existed, written out here (``_fgmres_loop``,
   ``_cfgmres_loop``) and not derived from the header: H after its rotations, cs, sn, g, the returned estimate and y, to 1e-13
   relative (complex values: of the modulus) -- the same IEEE operations in the same order, no FMA contraction on the x86-64
   baseline; what may differ by an ulp is the complex division (numpy: Smith's; the C++ run time: scaled) -- with the NaNs in the
   same places, part by part.  The operators between a real and a complex value are written component-wise, as C++ has them.
2. Against ``numpy.linalg.lstsq`` on Hessenberg matrices chosen well conditioned and diagonally dominant by rows: the entries
   above the diagonal uniform in [-1, 1] (both parts, complex) divided by m, the diagonal of modulus 2 with a random sign
   (phase), the subdiagonal -- the norms wn -- uniform in [0.25, 0.75]; beta uniform in [0.5, 2]; m in (1, 2, 3, 5, 8, 13, 20,
   30), three seeds each, both types: 48 cases.  The estimate is min |beta e1 - H y|, compared relative to beta (the minimum
   itself falls like 4^-m and lstsq's residual is formed by cancellation), y is the minimiser, compared in the 2-norm relative
   to |y|.  The bounds were not chosen in advance: the transcription's own largest deviation from lstsq over these 48 cases,
   measured on the CPU, is 3.0e-15 of beta for the estimate (m = 30, complex) and 5.9e-15 for y (m = 20, complex); the bounds
   are ten times those, 3.0e-14 and 5.9e-14.
The zero pivot of the ``den == 0`` case sits in the first column, where y is one division by zero, (inf, nan) in numpy and in
C++ alike; behind a later column y would go on through products of infinities, which C++ repairs by C99 Annex G and numpy does
not -- nothing of the class."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
LSTSQ_WORST = dict(estimate=3.0e-15, y=5.9e-15)                    # the transcription against lstsq, measured (the docstring)
LSTSQ_BOUND = {k: 10.0 * v for k, v in LSTSQ_WORST.items()}


# ---- the loops as they stood -----------------------------------------------------------------------------------------------------
def _fgmres_loop(m, cycles):
    """csrc/sns_krylov.hip, fgmres: from ``gv[0] = rn`` to the back-substitution, with the Gram-Schmidt results read from
    ``cycles`` = [(beta, [(h[0 .. j], wn), ...]), ...].  Returns the flat list the program prints."""
    f = np.float64
    H = [[f(0.0)] * (m + 1) for _ in range(m)]                     # H[j]: column j
    cs, sn, y, out = [f(0.0)] * m, [f(0.0)] * m, [f(0.0)] * m, []
    for beta, cols in cycles:
        gv = [f(0.0)] * (m + 1)
        gv[0] = f(beta)
        for j, (h, wn) in enumerate(cols):
            Hj = H[j]
            for k in range(j + 1):
                Hj[k] = f(h[k])
            Hj[j + 1] = f(wn)
            for k in range(j):                                     # previous rotations
                t0 = cs[k] * Hj[k] + sn[k] * Hj[k + 1]
                Hj[k + 1] = -sn[k] * Hj[k] + cs[k] * Hj[k + 1]
                Hj[k] = t0
            den = np.hypot(Hj[j], Hj[j + 1])
            cs[j] = Hj[j] / den if den > 0 else f(1.0)
            sn[j] = Hj[j + 1] / den if den > 0 else f(0.0)
            Hj[j] = den
            Hj[j + 1] = f(0.0)
            gv[j + 1] = -sn[j] * gv[j]
            gv[j] = cs[j] * gv[j]
            res = np.abs(gv[j + 1])
            out += [res, cs[j], sn[j]] + gv[:j + 2] + Hj[:j + 2]
        j = len(cols)
        for k in range(j - 1, -1, -1):
            sacc = gv[k]
            for q in range(k + 1, j):
                sacc = sacc - H[q][k] * y[q]
            y[k] = sacc / H[k][k]
        out += y[:j]
    return out


def _rz(r, z):
    """double * std::complex<double>: each part scaled."""
    return np.complex128(complex(r * z.real, r * z.imag))


def _cfgmres_loop(m, cycles):
    """csrc/sns_shifted.hip, cfgmres: the same stretch in complex arithmetic, rotations [cs, sn; -conj(sn), cs] with cs real."""
    f, c = np.float64, np.complex128
    H = [[c(0.0)] * (m + 1) for _ in range(m)]
    cs, sn, y, out = [f(0.0)] * m, [c(0.0)] * m, [c(0.0)] * m, []
    for beta, cols in cycles:
        gv = [c(0.0)] * (m + 1)
        gv[0] = c(complex(beta, 0.0))
        for j, (h, wn) in enumerate(cols):
            Hj, wn = H[j], f(wn)
            for k in range(j + 1):
                Hj[k] = c(h[k])
            Hj[j + 1] = c(complex(wn, 0.0))
            for k in range(j):
                t0 = _rz(cs[k], Hj[k]) + sn[k] * Hj[k + 1]
                Hj[k + 1] = -np.conj(sn[k]) * Hj[k] + _rz(cs[k], Hj[k + 1])
                Hj[k] = t0
            aa = np.abs(Hj[j])
            den = np.hypot(aa, wn)
            if den > 0.0 and aa > 0.0:
                cs[j] = aa / den
                sn[j] = _rz(wn / den, c(complex(Hj[j].real / aa, Hj[j].imag / aa)))
                Hj[j] = _rz(den / aa, Hj[j])
            else:
                cs[j] = f(0.0) if den > 0.0 else f(1.0)
                sn[j] = c(1.0) if den > 0.0 else c(0.0)
                Hj[j] = c(complex(wn, 0.0))
            Hj[j + 1] = c(0.0)
            gv[j + 1] = -np.conj(sn[j]) * gv[j]
            gv[j] = _rz(cs[j], gv[j])
            res = np.abs(gv[j + 1])
            out += [res, cs[j], sn[j]] + gv[:j + 2] + Hj[:j + 2]
        j = len(cols)
        for k in range(j - 1, -1, -1):
            sacc = gv[k]
            for q in range(k + 1, j):
                sacc = sacc - H[q][k] * y[q]
            y[k] = sacc / H[k][k]
        out += y[:j]
    return out


def _transcription(kind, m, cycles):
    with np.errstate(all="ignore"):
        return (_fgmres_loop if kind == "real" else _cfgmres_loop)(m, cycles)


# ---- the program -------------------------------------------------------------------------------------------------------------------
def _num(x):
    x = float(x)
    return "nan" if x != x else "inf" if x == float("inf") else "-inf" if x == -float("inf") else repr(x)


def _line(kind, m, cycles):
    words = [kind, str(m), str(len(cycles))]
    for beta, cols in cycles:
        words += [_num(beta), str(len(cols))]
        for h, wn in cols:
            for v in h:
                words += [_num(v)] if kind == "real" else [_num(complex(v).real), _num(complex(v).imag)]
            words.append(_num(wn))
    return " ".join(words)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("givens_lsq")
    exe, flags = str(tmp / "givens_lsq"), ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                          "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    # whether the toolchain has the sanitizer runtimes is asked of a trivial program; the test program itself must then build
    (tmp / "probe.cpp").write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(tmp / "probe.cpp"), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("toolchain without sanitizer runtimes")
    build = subprocess.run(flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"),
                                    os.path.join(ROOT, "tests", "givens_lsq_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]

    def go(cases):
        """cases: [(kind, m, cycles)] -> per case the program's numbers, shaped as the transcription's (real or complex each)."""
        r = subprocess.run([exe], input="".join(_line(*c) + "\n" for c in cases), capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        rows = r.stdout.split("\n")[:-1]
        assert len(rows) == len(cases)
        got = []
        for (kind, m, cycles), row in zip(cases, rows):
            words, want, vals = iter(row.split()), _transcription(kind, m, cycles), []
            for w in want:
                vals.append(np.complex128(complex(float(next(words)), float(next(words)))) if isinstance(w, np.complexfloating)
                            else np.float64(float(next(words))))
            assert next(words, None) is None, (kind, m, "more numbers than the transcription has")
            got.append((vals, want))
        return got
    return go


def _parts(vals):
    return np.array([p for v in vals for p in ((v.real, v.imag) if isinstance(v, np.complexfloating) else (v,))], dtype=np.float64)


def _same(got, want, what):
    """1e-13 relative, a complex value by its modulus; NaNs in the same places part by part; infinities equal."""
    g, w = _parts(got), _parts(want)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions", g, w)
    for a, b in zip(got, want):
        pa, pb = _parts([a]), _parts([b])
        fin = np.isfinite(pa) & np.isfinite(pb)
        assert np.array_equal(pa[~fin & ~np.isnan(pa)], pb[~fin & ~np.isnan(pb)]), (what, a, b)
        if fin.all():
            assert abs(a - b) <= 1e-13 * abs(b), (what, a, b)
        else:
            assert np.allclose(pa[fin], pb[fin], rtol=1e-13, atol=0.0), (what, a, b)


def _columns(rng, kind, n, scale=1.0):
    cols = []
    for j in range(n):
        h = rng.standard_normal(j + 1) * scale
        if kind == "cplx":
            h = h + 1j * rng.standard_normal(j + 1) * scale
        cols.append((list(h), abs(rng.standard_normal()) * scale))
    return cols


def _cases():
    rng = np.random.default_rng(4021)
    out = {}
    for kind in ("real", "cplx"):
        i = 1j if kind == "cplx" else 0.0
        out[kind, "m = 1"] = (1, [(2.0, [([0.75 - 0.5 * i], 1.25)])])
        out[kind, "early exit, 3 of 6 columns"] = (6, [(1.5, _columns(rng, kind, 3))])
        cols = _columns(rng, kind, 4)
        cols[3] = (cols[3][0], 0.0)
        out[kind, "wn == 0 at the last column"] = (5, [(0.7, cols)])
        out[kind, "Hjj == 0, wn > 0 at the first column"] = (3, [(1.0, [([0.0 * i], 0.5)] + _columns(rng, kind, 3)[1:])])
        # ... and at a later one: the first rotation is (cs, sn) = (0, 1) and leaves -h[0] = 0 on the diagonal
        out[kind, "Hjj == 0, wn > 0 at the second column"] = (3, [(1.0, [([0.0 * i], 2.0), ([0.0 * i, 3.0 + 2.0 * i], 0.25)])])
        out[kind, "den == 0"] = (2, [(1.0, [([0.0 * i], 0.0)])])
        cols = _columns(rng, kind, 4)
        cols[1][0][0] = NAN
        out[kind, "a NaN entry"] = (4, [(1.0, cols)])
        cols = _columns(rng, kind, 3)
        out[kind, "a NaN norm"] = (4, [(1.0, cols[:2] + [(cols[2][0], NAN)])])
        out[kind, "two cycles on one object, m = 3"] = (3, [(3.0, _columns(rng, kind, 3)), (0.25, _columns(rng, kind, 2))])
    return out


def test_against_the_loops_as_they_stood(run):
    cases = _cases()
    got = run([(kind, m, cycles) for (kind, _), (m, cycles) in cases.items()])
    for (kind, name), (vals, want) in zip(cases, got):
        _same(vals, want, (kind, name))
    by = {k: v[0] for k, v in zip(cases, got)}
    for kind in ("real", "cplx"):
        # the cases are what their names say: (res, cs, sn) lead each column's block
        assert by[kind, "Hjj == 0, wn > 0 at the first column"][1:3] == [0.0, 1.0]
        assert by[kind, "Hjj == 0, wn > 0 at the second column"][3 + 2 + 2:][1:3] == [0.0, 1.0]       # (behind the first column's block)
        assert by[kind, "den == 0"][:3] == [0.0, 1.0, 0.0] and not np.isfinite(_parts(by[kind, "den == 0"][-1:])).all()
        assert np.isnan(_parts(by[kind, "a NaN entry"])).any() and np.isnan(_parts(by[kind, "a NaN norm"])).any()
        assert by[kind, "wn == 0 at the last column"][7 + 9 + 11 + 2] == 0.0                          # sn of the fourth column


def test_seeded_sweep_against_the_loops(run):
    rng = np.random.default_rng(778)
    cases = []
    for kind in ("real", "cplx"):
        for _ in range(60):
            m = int(rng.integers(1, 31))
            cycles = [(float(rng.uniform(0.1, 10.0)), _columns(rng, kind, int(rng.integers(1, m + 1)), scale=float(rng.choice([1e-3, 1.0, 1e4]))))
                      for _ in range(int(rng.integers(1, 4)))]
            cases.append((kind, m, cycles))
    assert max(m for _, m, _ in cases) == 30
    for (kind, m, _), (vals, want) in zip(cases, run(cases)):
        _same(vals, want, (kind, m))


def _lstsq_cases():
    rng = np.random.default_rng(91)
    out = []
    for kind in ("real", "cplx"):
        for m in (1, 2, 3, 5, 8, 13, 20, 30):
            for _ in range(3):
                Hb = np.zeros((m + 1, m), dtype=complex if kind == "cplx" else float)
                for j in range(m):
                    up = rng.uniform(-1.0, 1.0, j) + (1j * rng.uniform(-1.0, 1.0, j) if kind == "cplx" else 0.0)
                    Hb[:j, j] = up / m
                    Hb[j, j] = 2.0 * (np.exp(2j * np.pi * rng.uniform()) if kind == "cplx" else rng.choice([-1.0, 1.0]))
                    Hb[j + 1, j] = rng.uniform(0.25, 0.75)
                out.append((kind, m, float(rng.uniform(0.5, 2.0)), Hb))
    return out


def _lstsq_deviation(vals, m, beta, Hb):
    """(the estimate's, y's) deviation of one run's numbers from numpy.linalg.lstsq."""
    rhs = np.zeros(m + 1, dtype=Hb.dtype)
    rhs[0] = beta
    y_ls = np.linalg.lstsq(Hb, rhs, rcond=None)[0]
    r_ls = np.linalg.norm(rhs - Hb @ y_ls)
    y = np.array(vals[-m:])
    res = float(vals[-m - (3 + 2 * (m + 1))])                       # the last column's block: res cs sn g[0 .. m] H[0 .. m]
    return abs(res - r_ls) / beta, float(np.linalg.norm(y - y_ls) / np.linalg.norm(y_ls))


def test_against_lstsq(run):
    cases = _lstsq_cases()
    scripted = [(kind, m, [(beta, [(list(Hb[:j + 1, j]), float(Hb[j + 1, j].real)) for j in range(m)])]) for kind, m, beta, Hb in cases]
    assert len(cases) == 48
    worst = dict(estimate=0.0, y=0.0, own_estimate=0.0, own_y=0.0)
    for (kind, m, beta, Hb), (vals, want) in zip(cases, run(scripted)):
        e, dy = _lstsq_deviation(vals, m, beta, Hb)
        oe, ody = _lstsq_deviation(want, m, beta, Hb)
        worst = dict(estimate=max(worst["estimate"], e), y=max(worst["y"], dy), own_estimate=max(worst["own_estimate"], oe),
                     own_y=max(worst["own_y"], ody))
    print("against lstsq: GivensLsq estimate %.3g y %.3g; the transcription's own estimate %.3g y %.3g; bounds %.3g %.3g"
          % (worst["estimate"], worst["y"], worst["own_estimate"], worst["own_y"], LSTSQ_BOUND["estimate"], LSTSQ_BOUND["y"]))
    assert worst["estimate"] <= LSTSQ_BOUND["estimate"] and worst["y"] <= LSTSQ_BOUND["y"]
