"""CPU check of where a chain reads its own data: data_view (csrc/mhx_stage.hpp) and DataView's
accessors (csrc/mhx_types.hpp) compiled on the CPU, against the definition in include/mhx.h:
mhx_set_dataset's arrays serve every walker; of mhx_set_dataset_planes walker c reads row c of
y [n_chains][n] and its sigma from sigma[n] (MHX_SIGMA_SHARED), sigma[c] (MHX_SIGMA_PER_CHAIN, and
the 1.0 the engine keeps per walker for MHX_SIGMA_NONE) or row c of sigma[n_chains][n]
(MHX_SIGMA_PER_POINT) - as the engine holds them: ys = y/sigma and w = 1/sigma, a plane's rows a
pitch apart.  Every array holds distinct integers, so an element names its place and a wrong one
cannot pass.  No device is touched."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
CHAINS, POINTS, PITCH = 3, 5, 7
# the bases of the arrays' values: element k of an array holds base + k
X0, X1, Y, W, PLANE_Y, PLANE_W = 1000, 2000, 3000, 4000, 5000, 6000

# "kind m0" (kind -1: the shared dataset, else a PlaneDesc::w_kind) answers, for every chain c and
# point i of the launch, "c i x0 x1 ys w" as the view reads them, then "pitches y_pitch w_pitch w_step"
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kPlaneWShared == 0 && kPlaneWScalar == 1 && kPlaneWPlane == 2, "the w_kinds");
  const int C = %(C)d, N = %(N)d, P = %(P)d;
  std::vector<double> x0(N), x1(N), y(N), w(N), py(C * P), pw(C * P);
  for (int k = 0; k < N; ++k) x0[k] = %(X0)d + k, x1[k] = %(X1)d + k, y[k] = %(Y)d + k, w[k] = %(W)d + k;
  for (int k = 0; k < C * P; ++k) py[k] = %(PLANE_Y)d + k, pw[k] = %(PLANE_W)d + k;
  int kind, m0, cols;
  while (scanf("%%d %%d %%d", &kind, &m0, &cols) == 3) {
    FnDesc f{};
    f.x = x0.data(), f.y = y.data(), f.w = w.data(), f.c = x1.data(), f.n = N, f.n_xcols = cols;
    PlaneDesc pd{};
    pd.y = py.data(), pd.w = pw.data(), pd.n_rows = C, pd.pitch = P, pd.w_kind = kind;
    if (kind >= 0) f.y = nullptr;                    // (what the planes replace must not be read)
    if (kind == kPlaneWScalar || kind == kPlaneWPlane) f.w = nullptr;
    const DataView v = data_view(f, kind >= 0 ? &pd : nullptr, m0);
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < N - m0; ++i)
        printf("%%d %%d %%.0f %%.0f %%.0f %%.0f\n", c, i, v.x0[i], v.x1 ? v.x1[i] : -1.0, v.y_row(c)[i],
               v.w_row(c)[(long long)i * v.w_step]);
    printf("pitches %%lld %%lld %%d\n", (long long)v.y_pitch, (long long)v.w_pitch, (int)v.w_step);
  }
  return 0;
}
''' % dict(C=CHAINS, N=POINTS, P=PITCH, X0=X0, X1=X1, Y=Y, W=W, PLANE_Y=PLANE_Y, PLANE_W=PLANE_W)

SHARED, W_SHARED, W_SCALAR, W_PLANE = -1, 0, 1, 2


def defined(kind, c, p):
    """(ys, w) of walker c at point p of the dataset, by include/mhx.h: the place in the arrays as
    the engine holds them (planes: rows PITCH apart; one sigma per walker: element c)"""
    ys = Y + p if kind == SHARED else PLANE_Y + c * PITCH + p
    w = {SHARED: W + p, W_SHARED: W + p, W_SCALAR: PLANE_W + c, W_PLANE: PLANE_W + c * PITCH + p}[kind]
    return ys, w


@pytest.fixture(scope="module")
def answers():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    tmp = tempfile.mkdtemp(prefix="mhx_dataview_")
    try:
        src, exe = os.path.join(tmp, "dataview_driver.cpp"), os.path.join(tmp, "dataview_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
        cases = [(kind, m0, cols) for kind in (SHARED, W_SHARED, W_SCALAR, W_PLANE) for m0 in (0, 2)
                 for cols in (1, 2)]
        out = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True,
                             check=True).stdout.split("\n")[:-1]
        got, at = {}, 0
        for kind, m0, cols in cases:
            rows = CHAINS * (POINTS - m0)
            got[kind, m0, cols] = ([[int(w) for w in line.split()] for line in out[at:at + rows]],
                                   [int(w) for w in out[at + rows].split()[1:]])
            at += rows + 1
        assert at == len(out)
        return got
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("kind", [SHARED, W_SHARED, W_SCALAR, W_PLANE])
@pytest.mark.parametrize("m0", [0, 2])
def test_every_chain_and_point_reads_the_element_the_definition_names(answers, kind, m0):
    for cols in (1, 2):
        rows, _ = answers[kind, m0, cols]
        assert [(r[0], r[1]) for r in rows] == [(c, i) for c in range(CHAINS) for i in range(POINTS - m0)]
        for c, i, x0, x1, ys, w in rows:
            p = m0 + i                                           # the point of the dataset
            assert (x0, x1) == (X0 + p, X1 + p if cols == 2 else -1), (c, i)
            assert (ys, w) == defined(kind, c, p), (c, i)
    # distinct values: no two (chain, point) of a per-walker array agree, so none can stand in for another
    if kind != SHARED:
        assert len({r[4] for r in rows}) == len(rows)


def test_the_pitches_and_steps_of_each_kind(answers):
    want = {SHARED: [0, 0, 1], W_SHARED: [PITCH, 0, 1], W_SCALAR: [PITCH, 1, 0], W_PLANE: [PITCH, PITCH, 1]}
    for (kind, m0, cols), (_, pitches) in answers.items():
        assert pitches == want[kind], (kind, m0)


def test_one_sigma_per_walker_does_not_move_with_the_first_point(answers):
    """the scalar 1/sigma of walker c is element c whatever m0 is: offset by m0 it would be walker
    c + m0's"""
    for cols in (1, 2):
        w0 = {(r[0]): r[5] for r in answers[W_SCALAR, 0, cols][0]}
        w2 = {(r[0]): r[5] for r in answers[W_SCALAR, 2, cols][0]}
        assert w0 == w2 == {c: PLANE_W + c for c in range(CHAINS)}
        assert all(r[5] == PLANE_W + r[0] for m0 in (0, 2) for r in answers[W_SCALAR, m0, cols][0])
