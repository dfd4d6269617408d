// emi_biper_body.h -- biperiodicisation of limited-area grid fields: the kernels of FPBIPERE and ETIBIHIE (etrans/cpu/biper:
// espline_mod.F90, esmoothe_mod.F90, ewindowe_mod.F90).  Included from emi_kernels_body.h, so it is compiled once per precision
// (real_t) and by the CPU emulator.
//
// One layout serves both routines: element (x, f, y), zero-based, of the fields lies at w[x + f * sf + y * sy] --
// FPBIPERE's PGPBI(KD1, KNUBI): sf = KD1, sy = KDLON; ETIBIHIE's PGPBI(KSTART:KDLSM, KNUBI, KDGL): sf = row length, sy = KNUBI rows,
// w advanced to x = 1.  All offsets are 64-bit.  Every kernel keeps the reference's order of operations and forms no fused
// multiply-add (EMI_FP_STRICT), so the results are the reference's bytes; the kernels move far more bytes than they compute on.

// The cubic that continues a line known on 1 .. u over u + 1 .. n (espline_mod.F90:137-154 with PALFA = 0: the ZNY terms are
// x - 0 * finite and change no bit).  v1, v2, vu, vum1 = v(1), v(2), v(u), v(u - 1); k = n - u + 1; lam = kx / (kx + 1) of the x direction
// in BOTH passes, as espline_mod.F90:179-181 has it.
struct BiperCubic {
  real_t a, b, c, d;
};
EMI_DEVFN BiperCubic biper_cubic(real_t v1, real_t v2, real_t vu, real_t vum1, int ik, real_t lam) {
  EMI_FP_STRICT();
  const real_t k = (real_t)ik, kp1 = k + (real_t)1;
  const real_t ea = ((v1 - vu) / k - vu + vum1) * (real_t)6 / kp1;
  const real_t eb = (v2 - v1 - (v1 - vu) / k) * (real_t)6 / kp1;
  const real_t mm = (real_t)4 - lam * lam;
  const real_t m1 = ((real_t)2 * ea - lam * eb) / mm, m2 = ((real_t)2 * eb - lam * ea) / mm;
  BiperCubic q;
  q.a = vu;
  q.b = (v1 - vu) / k - ((real_t)2 * m1 + m2) * k / (real_t)6;
  q.c = (real_t)0.5 * m1;
  q.d = (m2 - m1) / ((real_t)6 * k);
  return q;
}
EMI_DEVFN real_t biper_lambda(int kx) {
  EMI_FP_STRICT();
  const real_t k = (real_t)kx;
  return k / (k + (real_t)1);
}

// x pass: rows 0 .. nrows - 1 of every field, columns UX .. X - 1.  One thread per (j, row, field), j fastest: consecutive lanes
// write consecutive x; the four values of the row that make the coefficients are broadcast reads.
EMI_KERNEL_LB(256) void k_biper_spline_x(real_t *w, long long sf, long long sy, int X, int UX, int nrows, int nf) {
  EMI_FP_STRICT();
  const int E = X - UX;
  const long long id = (long long)EMI_BID * 256 + EMI_TID;
  if (id >= (long long)E * nrows * nf) return;
  const int j = (int)(id % E) + 1;
  const long long r = id / E;
  const int y = (int)(r % nrows), f = (int)(r / nrows);
  real_t *row = w + f * sf + y * sy;
  const BiperCubic q = biper_cubic(row[0], row[1], row[UX - 1], row[UX - 2], E + 1, biper_lambda(E + 1));
  const real_t zj = (real_t)j;
  row[UX - 1 + j] = q.a + zj * (q.b + zj * (q.c + q.d * zj));
}

// y pass: columns 0 .. ncols - 1 of every field, rows UY .. Y - 1.  One thread per (x, field), x fastest (contiguous); the thread
// keeps the coefficients of its column in registers and walks j.
EMI_KERNEL_LB(256) void k_biper_spline_y(real_t *w, long long sf, long long sy, int ncols, int Y, int UY, int kx, int nf) {
  EMI_FP_STRICT();
  const long long id = (long long)EMI_BID * 256 + EMI_TID;
  if (id >= (long long)ncols * nf) return;
  const int x = (int)(id % ncols), f = (int)(id / ncols);
  real_t *col = w + f * sf + x;
  const BiperCubic q = biper_cubic(col[0], col[sy], col[(UY - 1) * sy], col[(UY - 2) * sy], Y - UY + 1, biper_lambda(kx));
  for (int j = 1; j <= Y - UY; j++) {
    const real_t zj = (real_t)j;
    col[(UY - 1 + j) * sy] = q.a + zj * (q.b + zj * (q.c + zj * q.d));
  }
}

// One half-pass of ESMOOTHE (esmoothe_mod.F90:137-146 | 164-173) over all fields: the points x0 <= x < x0 + nx, y0 <= y < y0 + ny are
// smoothed from the field as it stands (the stencil wraps with the periods X and Y) into the dense band buffer
// band[f][y - y0][x - x0]; nothing in w is written, so no workgroup reads what another one writes.  k_biper_copy then puts the band
// back.  Only the band and its one-point halo are touched.
EMI_KERNEL_LB(256) void k_biper_smooth(const real_t *w, long long sf, long long sy, int X, int Y, int x0, int nx, int y0, int ny, int nf, real_t *band) {
  EMI_FP_STRICT();
  const long long id = (long long)EMI_BID * 256 + EMI_TID;
  if (id >= (long long)nx * ny * nf) return;
  const int ix = (int)(id % nx);
  const long long r = id / nx;
  const int iy = (int)(r % ny), f = (int)(r / ny);
  const int x = x0 + ix, y = y0 + iy;
  const int xp = x + 1 == X ? 0 : x + 1, xm = x == 0 ? X - 1 : x - 1;
  const int yp = y + 1 == Y ? 0 : y + 1, ym = y == 0 ? Y - 1 : y - 1;
  const real_t *z = w + f * sf;
  const real_t *zc = z + y * sy, *zu = z + yp * sy, *zd = z + ym * sy;
  const real_t s = ((real_t)4 * zc[x] + (real_t)2 * (zc[xp] + zc[xm] + zu[x] + zd[x]) + zu[xp] + zu[xm] + zd[xp] + zd[xm]) / (real_t)16;
  band[id] = s;
}

// dst[x + f * dsf + y * dsy] = src[x + f * ssf + y * ssy], x < nx, y < ny, f < nf: the band of a half-pass back into the field, and
// the C+I part of packed fields (FPBIPERE with LDZON = .FALSE.) into a scratch copy and back out at the row stride KDLON.
EMI_KERNEL_LB(256) void k_biper_copy(real_t *dst, long long dsf, long long dsy, const real_t *src, long long ssf, long long ssy, int nx, int ny, int nf) {
  const long long id = (long long)EMI_BID * 256 + EMI_TID;
  if (id >= (long long)nx * ny * nf) return;
  const int x = (int)(id % nx);
  const long long r = id / nx;
  const int y = (int)(r % ny), f = (int)(r / ny);
  dst[x + f * dsf + y * dsy] = src[x + f * ssf + y * ssy];
}

// Boyd's window (ewindowe_mod.F90:141-166) on fields of ny rows of ld points, field stride sf.  dir = 0, the x blend:
// w(X + j) = bx(j) w(j) + (1 - bx(j)) w(X + j) on every row, j = 1 .. nw (n1 = ny rows, P = X); dir = 1, the y blend: the same between
// rows j and Y + j over all n1 = ld columns (P = Y).  The two are separate launches, x first: the y blend reads what the x blend wrote.
EMI_KERNEL_LB(256) void k_biper_boyd(real_t *w, long long sf, int ld, int dir, int P, int nw, int n1, int nf, const real_t *b) {
  EMI_FP_STRICT();
  const long long id = (long long)EMI_BID * 256 + EMI_TID;
  const long long per = (long long)nw * n1;
  if (id >= per * nf) return;
  const int f = (int)(id / per);
  const long long r = id - f * per;
  real_t *z = w + f * sf;
  long long lo, hi;
  int j;
  if (dir == 0) {
    j = (int)(r % nw);
    const long long row = r / nw;
    lo = row * ld + j, hi = row * ld + P + j;
  } else {
    const int x = (int)(r % n1);
    j = (int)(r / n1);
    lo = (long long)j * ld + x, hi = (long long)(P + j) * ld + x;
  }
  const real_t bj = b[j];
  z[hi] = bj * z[lo] + ((real_t)1 - bj) * z[hi];
}
