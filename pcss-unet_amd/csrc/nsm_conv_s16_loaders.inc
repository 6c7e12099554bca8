// Operand descriptions of the 16-bit GEMMs and their LDS-DMA loaders
// (ConvActDma, RowsKDma, PixRowsDma: the images nsm_conv_s16_dma.inc describes).
// They move raw 16-bit words, so they do not depend on the format, but the
// kernels are named after them, so they stay inside the format namespace:
// included by nsm_conv_s16.inc (in nsm_bf and in nsm_h) and, in nsm_bf, at the
// top of nsm_conv_h2.hip, whose direct 3x3 convolution reads h2 tensors through
// the bf16 loaders (nsm_conv_h2d.inc). Needs nsm_conv.h.

struct ConvActPB {  // im2col of NHWC bf16 activations; K = (tap, channel)
  const bf16_t* x;
  int ld, cin, H, W, M, ksize, K;
  FastDiv fdW, fdH, fdC;
  const float* scale;
  const float* shift;
  const float* mask;
  int mask_ld, mask_on;
  float slope;
  int cm;  // LDS-DMA 3x3: channel-major K-tile order (see ConvActDma::prep)
};

struct RowsKPB {  // dense bf16 rows [nrows][ldw], K valid columns
  const bf16_t* w;
  int ldw, nrows, K;
  int cin, cm;  // LDS-DMA 3x3: channel-major K-tile order (see ConvActDma::prep)
};

struct PixRowsPB {  // rows = pixels (the wgrad K), columns = bf16 channels
  const bf16_t* x;
  int ld, ncols, cin, H, W, M, ksize;
  FastDiv fdW, fdH;
  const float* scale;
  const float* shift;
  const float* mask;
  int mask_ld, mask_on;
  float slope;
};


// ---- MK loaders (forward / dgrad) --------------------------------------------
template <int R, int NW, int BK = DBK>
struct ConvActDma {  // im2col rows of NHWC bf16 activations (one tap per K-tile)
  static constexpr bool KM = false;
  static constexpr int CH = BK / 8, RPI = 64 / CH;  // 16-B chunks per row, rows per DMA
  static constexpr int NI = R / (RPI * NW);         // DMA instructions per wave and K-tile
  static_assert(NI >= 1 && NI * RPI * NW == R, "dma shape");
  using P = ConvActPB;
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t base[NI];  // byte offset of (pixel row, swizzled chunk) at tap shift 0
  int py[NI], px[NI];
  int tdy, tdx, toff;  // current K-tile: tap offsets and its byte offset

  __device__ void init(const P& p, int m0, int, int, int wid, int lane) {
    const int base_pix = max(0, m0 - p.W - 1);
    rsrc = make_rsrc_b(p.x + (size_t)base_pix * p.ld, (long long)(p.M - base_pix) * p.ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (wid * NI + i) * RPI + lane / CH;
      int q = m0 + row;
      const bool v = q < p.M;
      q = v ? q : 0;
      const int t = (int)fdiv((uint32_t)q, p.fdW);
      const int xx = q - t * p.W;
      const int b = (int)fdiv((uint32_t)t, p.fdH);
      const int yy = t - b * p.H;
      base[i] = (uint32_t)((q - base_pix) * p.ld + ((lane % CH) ^ dswz<BK>(row)) * 8) * 2u;
      px[i] = xx;
      py[i] = v ? yy : -0x40000000;
    }
  }
  __device__ void prep(const P& p, int k0) {
    int tap, c0;
    if (p.cm) {  // K-tile t = (channel chunk j, tap): k0 = (j * 9 + tap) * BK
      const int t = k0 / BK, j = t / 9;
      tap = t - j * 9;
      c0 = j * BK;
    } else {     // tap-major: k0 = tap * cin + c0
      tap = (int)fdiv((uint32_t)k0, p.fdC);
      c0 = k0 - tap * p.cin;
    }
    tdy = tdx = 0;
    if (p.ksize == 3) {
      tdy = tap / 3 - 1;
      tdx = tap - (tap / 3) * 3 - 1;
    }
    toff = ((tdy * p.W + tdx) * p.ld + c0) * 2;
  }
  __device__ void one(const P& p, const bf16_t* stage, int wid, int i) const {
    const int yy = py[i] + tdy, xx = px[i] + tdx;
    const bool ok = ((unsigned)yy < (unsigned)p.H) & ((unsigned)xx < (unsigned)p.W);
    // (a halo row's offset may wrap negative: it carries the OOB bit anyway)
    dma16(rsrc, stage + (wid * NI + i) * 512, (base[i] + (uint32_t)toff) | (ok ? 0u : OOB));
  }
};

template <int R, int NW, int BK = DBK>
struct RowsKDma {  // dense bf16 rows [nrows][ldw] (packed weights)
  static constexpr bool KM = false;
  static constexpr int CH = BK / 8, RPI = 64 / CH;
  static constexpr int NI = R / (RPI * NW);
  static_assert(NI >= 1 && NI * RPI * NW == R, "dma shape");
  using P = RowsKPB;
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t base[NI];
  uint32_t koff;

  __device__ void init(const P& p, int n0, int, int, int wid, int lane) {
    rsrc = make_rsrc_b(p.w + (size_t)n0 * p.ldw, (long long)(p.nrows - n0) * p.ldw);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (wid * NI + i) * RPI + lane / CH;
      base[i] = ((uint32_t)(row * p.ldw + ((lane % CH) ^ dswz<BK>(row)) * 8) * 2u) |
                (n0 + row < p.nrows ? 0u : OOB);
    }
  }
  __device__ void prep(const P& p, int k0) {
    int k = k0;
    if (p.cm) {  // the packed weights stay [n][tap][cin]: same K-tile as ConvActDma
      const int t = k0 / BK, j = t / 9;
      k = (t - j * 9) * p.cin + j * BK;
    }
    koff = (uint32_t)k * 2u;
  }
  __device__ void one(const P&, const bf16_t* stage, int wid, int i) const {
    dma16(rsrc, stage + (wid * NI + i) * 512, base[i] + koff);
  }
};

// ---- KM loader (weight gradient): pixel rows of one operand -------------------
template <int R, int NW, bool SHIFT, int BK = DBK>
struct PixRowsDma {
  static constexpr bool KM = true;
  static constexpr int RB = 2 * R;                 // bytes per pixel row
  static constexpr int NI = BK * RB / 1024 / NW;   // DMA instructions per wave and K-tile
  static_assert(R >= 32 && NI >= 1 && NI * NW * 1024 == BK * RB, "dma shape");
  using P = PixRowsPB;
  __amdgpu_buffer_rsrc_t rsrc;
  // per instruction: pixel row in the K-tile, channel, and (shifted operand)
  // its tap: a tile may span several taps when R > Cin (meta = colok<<4 |
  // (dy+1)<<2 | (dx+1))
  int row[NI], cof[NI], meta[NI];
  int base_pix, kend, k0;

  __device__ void init(const P& p, int off, int kbeg, int kend_, int wid, int lane) {
    kend = kend_;
    base_pix = max(0, kbeg - p.W - 1);
    rsrc = make_rsrc_b(p.x + (size_t)base_pix * p.ld, (long long)(p.M - base_pix) * p.ld);
    const int taps = p.ksize * p.ksize;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int byte = (wid * NI + i) * 1024 + lane * 16;
      const int k = byte / RB, pc = (byte % RB) / 16;
      row[i] = k;
      const int col = off + ((pc ^ kmswz<R>(k)) << 3);  // column of the GEMM's N (or M)
      int tap = 0, c = col;
      if (p.cin > 0) {
        tap = col / p.cin;
        c = col - tap * p.cin;
      }
      cof[i] = c;
      int dy = 0, dx = 0;
      if (SHIFT && p.ksize == 3) {
        dy = tap / 3 - 1;
        dx = tap % 3 - 1;
      }
      const bool ok = c < p.ncols && (p.cin == 0 || tap < taps);
      meta[i] = (ok ? 16 : 0) | ((dy + 1) << 2) | (dx + 1);
    }
  }
  __device__ void prep(const P&, int k0_) { k0 = k0_; }
  __device__ void one(const P& p, const bf16_t* stage, int wid, int i) const {
    const int q = k0 + row[i];
    const int m = meta[i];
    bool ok = (m >> 4) & (q < kend);
    int src = q;
    if constexpr (SHIFT) {
      const int dy = ((m >> 2) & 3) - 1, dx = (m & 3) - 1;
      const int t = (int)fdiv((uint32_t)q, p.fdW);
      const int xx = q - t * p.W;
      const int b = (int)fdiv((uint32_t)t, p.fdH);
      const int yy = t - b * p.H;
      ok = ok & ((unsigned)(yy + dy) < (unsigned)p.H) & ((unsigned)(xx + dx) < (unsigned)p.W);
      src = q + dy * p.W + dx;
    }
    const uint32_t off = ((uint32_t)((src - base_pix) * p.ld + cof[i]) * 2u) | (ok ? 0u : OOB);
    dma16(rsrc, stage + (wid * NI + i) * 512, off);
  }
};
