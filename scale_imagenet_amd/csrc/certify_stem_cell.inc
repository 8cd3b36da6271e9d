// One pooled cell of stage 0 for one channel, included where a kernel needs it: in scope are STEM_AT(k, c, r, q) = the centre
// (k = 0) / radius (k = 1) of channel c at row r, column q of the cell's 5 x 5 field (in LDS), the channel's weights
// double wr[27], its bias b, the folded BatchNorm sc, sh and the slack sl; it leaves lo_bit and hi_bit.  The nine convolution
// outputs of the cell: a field row is read once (all 64 lanes of a wave read the same address: a broadcast) and feeds every
// output it belongs to; the tap order of va_stem_patch.  ttnet_certify_u8's stage 0 and the patch sweep both include it, so a
// cell has the same bits whoever computes it.  (Text, not a function: as an inlined function the same lines cost
// certify_stem_kernel 183 VGPRs instead of 130.)
  double mid[3][3], rad[3][3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) mid[dy][dx] = rad[dy][dx] = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      double xc[5], xr[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        xc[q] = STEM_AT(0, c, r, q);
        xr[q] = STEM_AT(1, c, r, q);
      }
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int kh = r - dy;
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const double wv = wr[(c * 3 + kh) * 3 + kw];
            mid[dy][dx] = fma(wv, xc[dx + kw], mid[dy][dx]);
            rad[dy][dx] = fma(fabs(wv), xr[dx + kw], rad[dy][dx]);
          }
      }
    }
  double best_lo = -INFINITY, best_hi = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const double lo = fmax(mid[dy][dx] - rad[dy][dx] + b, 0.0), hi = fmax(mid[dy][dx] + rad[dy][dx] + b, 0.0);   // ReLU
      const double ylo = (sc >= 0.0 ? lo : hi) * sc + sh, yhi = (sc >= 0.0 ? hi : lo) * sc + sh;   // a negative scale swaps the bounds
      best_lo = fmax(best_lo, ylo);                                  // MaxPool2d(3): max of the lows, max of the highs
      best_hi = fmax(best_hi, yhi);
    }
  const bool lo_bit = best_lo - sl >= 0.0;
  const bool hi_bit = (best_hi + sl >= 0.0) || lo_bit;                          // (lo_bit <= hi_bit whatever the arithmetic did)
