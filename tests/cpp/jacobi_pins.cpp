// jacobi_pins.cpp -- the seven eigen / SVD routines of the solver math under their public names, bit for bit: reads cases
// (tests/golden/jacobi_pins.txt, written by tools/gen_jacobi_pins.py), writes every output as the 64-bit pattern of each
// binary64 value.  Build with -O2 -ffp-contract=off, as the *_math_cpu programs.
//   jacobi_pins <cases> <out>
// A case is one line `case <routine> <name> <m> <count> <hex> ...`; every other line is skipped.  The answer is one line
// `out <hex> ...` per case, in order.
//   tri   16 values: a (4 x 4 row-major)                      -> x[4]
//   sim3  16 values: a (symmetric 4 x 4)                      -> q[4]
//   null9 144 values: the 16 rows of A (V = I is added here)   -> nv[9]   (init_null_vector with InitHostLanes)
//   rank2 9 values: Fpre                                      -> Fn[9]
//   svd3  9 values: A                                         -> U[9] w[3] V[9]
//   ls6   6 m + 6 values: la (6 x m row-major), rho           -> lx[m]
//   eig12 144 values: a (symmetric 12 x 12)                   -> ut[4][12] d[12]
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "initializer_math.h"
#include "initializer_reconstruct_math.h"
#include "pnp_math.h"
#include "sim3_math.h"
#include "triangulate_math.h"

using namespace orbfe;

static double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: jacobi_pins <cases> <out>\n"); return 2; }
  FILE* fi = fopen(argv[1], "r");
  FILE* fo = fopen(argv[2], "w");
  if (!fi || !fo) { fprintf(stderr, "jacobi_pins: cannot open a file\n"); return 2; }
  static PnpWork W;
  char word[64], routine[64], name[64];
  while (fscanf(fi, "%63s", word) == 1) {
    if (strcmp(word, "case") != 0) {  // an `out` line or a comment: skip to the end of the line
      int ch;
      while ((ch = fgetc(fi)) != EOF && ch != '\n') {}
      continue;
    }
    int m = 0, count = 0;
    if (fscanf(fi, "%63s %63s %d %d", routine, name, &m, &count) != 4) { fprintf(stderr, "jacobi_pins: bad case line\n"); return 2; }
    std::vector<double> in(count), out;
    for (int i = 0; i < count; i++) {
      unsigned long long b;
      if (fscanf(fi, "%llx", &b) != 1) { fprintf(stderr, "jacobi_pins: %s: short input\n", name); return 2; }
      in[i] = from_bits(b);
    }
    const std::string r = routine;
    const int want = r == "tri" || r == "sim3" ? 16 : r == "null9" ? 144 : r == "rank2" || r == "svd3" ? 9 : r == "ls6" ? 6 * m + 6
                   : r == "eig12" ? 144 : -1;
    if (want != count || (r == "ls6" && (m < 3 || m > 5))) { fprintf(stderr, "jacobi_pins: %s %s: bad size\n", routine, name); return 2; }
    if (r == "tri") {
      double a[16], x[4];
      for (int i = 0; i < 16; i++) a[i] = in[i];
      tri_null_vector(a, x);
      out.assign(x, x + 4);
    } else if (r == "sim3") {
      double a[16], q[4];
      for (int i = 0; i < 16; i++) a[i] = in[i];
      sim3_top_eigenvector(a, q);
      out.assign(q, q + 4);
    } else if (r == "null9") {
      double mm[kInitRows][9], nv[9];
      for (int i = 0; i < kInitRows; i++)
        for (int j = 0; j < 9; j++) mm[i][j] = i < kInitARows ? in[9 * i + j] : (i - kInitARows == j ? 1.0 : 0.0);
      const InitHostLanes ln;
      init_null_vector(ln, mm, nv);
      out.assign(nv, nv + 9);
    } else if (r == "rank2") {
      double Fn[9];
      init_rank2(in.data(), Fn);
      out.assign(Fn, Fn + 9);
    } else if (r == "svd3") {
      double U[9], w[3], V[9];
      recon_svd3(in.data(), U, w, V);
      out.assign(U, U + 9);
      out.insert(out.end(), w, w + 3);
      out.insert(out.end(), V, V + 9);
    } else if (r == "ls6") {
      for (int i = 0; i < 6 * m; i++) W.la[i] = in[i];
      for (int i = 0; i < 6; i++) W.rho[i] = in[6 * m + i];
      pnp_ls6(&W, m);
      out.assign(W.lx, W.lx + m);
    } else {
      for (int i = 0; i < 144; i++) W.a[i] = in[i];
      pnp_eig12(&W);
      for (int k = 0; k < 4; k++) out.insert(out.end(), W.ut[k], W.ut[k] + 12);
      out.insert(out.end(), W.d, W.d + 12);
    }
    fprintf(fo, "out");
    for (double d : out) fprintf(fo, " %016llx", (unsigned long long)to_bits(d));
    fprintf(fo, "\n");
  }
  fclose(fi);
  fclose(fo);
  return 0;
}
