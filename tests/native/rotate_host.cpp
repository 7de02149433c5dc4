// Host run of the shipped rotation order (nlml_hpe_amd/csrc/rotate_ref.h, the statement the kernel compiles) for
// tests/test_rotation_host.py, which builds it with -fsanitize=address,undefined: the grid and the per-face functions over a few
// thousand cells on exactly sized heap buffers, checking invariants that need no reference --
//   the copy rule            the zero cell is the base bit for bit (its f64 form the same values widened), whichever bins are named
//   identity matrices        a cell rotated by Rx(0), Ry(0), Rz(0) -- with the -0.0 entries numpy puts there -- is the base up to the
//                            sign of a zero, and every -0.0 coordinate comes out +0.0
//   zero matrices            the fma(a, 0, +0.0) chains give +0.0 exactly, for every finite input of either sign
//   grid == per face         the grid cell (id, y, p, r) equals the per-face call with that cell's three matrices
//   out == (float)out64      one rounding
// Prints "rotate host ok" and returns 0, or says what failed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../nlml_hpe_amd/csrc/rotate_ref.h"

using namespace nlml;

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // [0, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg_state >> 11) * (1.0 / 9007199254740992.0);
}

static uint32_t bits32(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t bits64(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

// the axis layouts of IntrinsicRotation.py:90-105 from a cosine and a sine (no trigonometry is under test here)
static void axis_matrix(char axis, double c, double s, double* M) {
  const double rx[9] = {1, 0, 0, 0, c, -s, 0, s, c}, ry[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
  memcpy(M, axis == 'x' ? rx : axis == 'y' ? ry : rz, sizeof rx);
}

static int fail(const char* what, long long where) {
  printf("FAILED: %s at %lld\n", what, where);
  return 1;
}

int main() {
  const int64_t I = 5;
  const int ny = 11, np = 9, nr = 7, zy = 5, zp = 4, zr = 3;   // 3,465 cells
  const int64_t rows = I * ny * np * nr;
  std::vector<float> base((size_t)I * RT_F), out((size_t)rows * RT_F), out_face(RT_F);
  std::vector<double> out64((size_t)rows * RT_F), out64_face(RT_F), ryaw(9 * ny), rpitch(9 * np), rroll(9 * nr);
  for (size_t e = 0; e < base.size(); ++e) base[e] = (float)(uniform() * 4.0 - 2.0) * (e % 5 == 0 ? 320.0f : 1.0f);
  for (int64_t id = 0; id < I; ++id) {
    float* b = base.data() + id * RT_F;
    b[0] = -0.0f; b[4] = 0.0f; b[3 * 300] = b[3 * 300 + 1] = b[3 * 300 + 2] = -0.0f; b[RT_F - 1] = -0.0f;
  }
  auto fill = [](std::vector<double>& t, int n, int zero, char axis) {
    for (int k = 0; k < n; ++k) {
      const double a = k == zero ? 0.0 : uniform() * 6.0 - 3.0;
      axis_matrix(axis, k == zero ? 1.0 : cos(a), k == zero ? 0.0 : sin(a), t.data() + 9 * k);
    }
  };
  fill(ryaw, ny, zy, 'y');
  fill(rpitch, np, zp, 'x');
  fill(rroll, nr, zr, 'z');

  for (int order = 0; order < 2; ++order) {
    rt_grid_host(base.data(), I, ryaw.data(), ny, rpitch.data(), np, rroll.data(), nr, order, zy, zp, zr, out.data(), out64.data());
    int64_t row = 0;
    for (int64_t id = 0; id < I; ++id)
      for (int y = 0; y < ny; ++y)
        for (int p = 0; p < np; ++p)
          for (int r = 0; r < nr; ++r, ++row) {
            const float* o = out.data() + row * RT_F;
            const double* o64 = out64.data() + row * RT_F;
            const float* b = base.data() + id * RT_F;
            for (int e = 0; e < RT_F; ++e)
              if (bits32(o[e]) != bits32((float)o64[e])) return fail("out is not one rounding of out64", row);
            if (y == zy && p == zp && r == zr) {
              for (int e = 0; e < RT_F; ++e)
                if (bits32(o[e]) != bits32(b[e]) || bits64(o64[e]) != bits64((double)b[e])) return fail("copy rule", row);
              continue;
            }
            const double *M0, *M1, *M2;
            rt_cell_order(order, ryaw.data() + 9 * y, rpitch.data() + 9 * p, rroll.data() + 9 * r, M0, M1, M2);
            rt_face_host(b, M0, M1, M2, out_face.data(), out64_face.data());
            if (memcmp(o, out_face.data(), RT_F * sizeof(float)) || memcmp(o64, out64_face.data(), RT_F * sizeof(double)))
              return fail("grid cell differs from the per-face call", row);
          }
    // the same grid with no zero bin named: the (zy, zp, zr) cell is rotated by three identity matrices
    rt_grid_host(base.data(), I, ryaw.data(), ny, rpitch.data(), np, rroll.data(), nr, order, -1, -1, -1, out.data(), nullptr);
    for (int64_t id = 0; id < I; ++id) {
      const float* o = out.data() + (((id * ny + zy) * np + zp) * nr + zr) * RT_F;
      const float* b = base.data() + id * RT_F;
      for (int e = 0; e < RT_F; ++e) {
        if (o[e] != b[e]) return fail("identity rotation changed a value", id * RT_F + e);
        if (b[e] == 0.0f && bits32(o[e]) != 0u) return fail("identity rotation left a -0.0", id * RT_F + e);
        if (b[e] != 0.0f && bits32(o[e]) != bits32(b[e])) return fail("identity rotation changed a non-zero's bits", id * RT_F + e);
      }
    }
  }

  // zero matrices: fma(a, 0, +0.0) = +0.0 for every finite a, of either sign
  const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  rt_face_host(base.data(), Z, Z, Z, out_face.data(), out64_face.data());
  for (int e = 0; e < RT_F; ++e)
    if (bits32(out_face[e]) != 0u || bits64(out64_face[e]) != 0ull) return fail("zero matrices: not +0.0", e);
  // either output alone
  rt_face_host(base.data(), ryaw.data(), rpitch.data(), rroll.data(), out_face.data(), nullptr);
  rt_face_host(base.data(), ryaw.data(), rpitch.data(), rroll.data(), nullptr, out64_face.data());
  for (int e = 0; e < RT_F; ++e)
    if (bits32(out_face[e]) != bits32((float)out64_face[e])) return fail("out alone / out64 alone disagree", e);
  // an empty grid touches nothing
  rt_grid_host(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0, -1, -1, -1, nullptr, nullptr);

  printf("rotate host ok: %lld cells, both orders\n", (long long)rows);
  return 0;
}
