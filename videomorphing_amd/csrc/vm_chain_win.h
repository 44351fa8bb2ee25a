// vm_chain_win.h -- the window form of the compositor's chain (vm_chain.h), stated once as the statements a window kernel
// includes at the top of its body -- k_render_win (vm_render.hip), k_warp_win (vm_warp.hip) and k_motion_win (vm_carry.hip) -- or of its sample loop's
// (k_shutter_win, vm_shutter.hip; k_tblur_win, vm_tshutter.hip; k_viewport_win, vm_viewport.hip; k_vblur_win,
// vm_vshutter.hip, with the hooks of all three).  It is no function because
// the compiler lays a kernel out differently once this body sits behind any function boundary, a lambda included (the
// fallback's float2 gathers stay whole, the vectoriser pairs other operations, and the sum after the inside / outside
// split of the tap is emitted once instead of once per side): k_warp_win<true, CANVAS, true> lost 1.5 us of 100 that way.
// Included like this every window kernel keeps the loop it had when each unit carried its own copy.
//
// In scope where it is included: constexpr bool HAS_U, RATES; int w, h, rs, tiles_x, ntiles; float geo_fa;
// const float2 *vf, *uf, *rates (rates is read only if RATES, and only through rate_at: vm_tshutter.hip puts a Ramped of
// vm_ramp.h there); namespace vm_chain.  It leaves int x, y (the pixel) and
// Landing L, and returns from the kernel for a thread without a pixel (the whole workgroup past the last tile, or a
// pixel outside the image -- after the barrier).  Everything else stays inside its block.
//
// A kernel that walks the chain several times in a loop (vm_shutter.hip) defines, before it includes this,
//   VM_CHAIN_WIN_NO_PIXEL        what a thread without a pixel does after the barrier (default: return; in a loop the
//                                thread has to stay for the barriers of the rounds to come)
//   VM_CHAIN_WIN_STAGE(ox, oy)   whether the window is staged at (ox, oy), workgroup-uniform (default: true; in a loop
//                                the barrier before a restaging belongs to it, and a window that has not moved may stay)
//   VM_CHAIN_WIN_STAGE_FIELD     whether a staging copies v and u, workgroup-uniform (default: true; vm_tshutter.hip stages
//                                the rates at every sample, v and u only where the window has moved)
// A kernel whose output grid is not the field's (vm_viewport.hip: x, y, tiles_x and ntiles then count OUTPUT pixels and
// tiles, w, h and rs stay the field's) defines, by including vm_viewport_win.h,
//   VM_CHAIN_WIN_Q_X, _Q_Y           the point q of the halfway domain the chain of output pixel (x, y) starts from
//                                    (default: (float)x, (float)y, the pixel's centre)
//   VM_CHAIN_WIN_ORIGIN_X, _Y        the field cell the tile's footprint begins at, from which the window is placed
//   VM_CHAIN_WIN_CENTRE_X, _Y        and the cell at its centre, within the field, whose warp displaces the window
//                                    (defaults: bx, by and min(bx + RW / 2, wm1), min(by + RH / 2, hm1): the tile itself)
//   VM_CHAIN_WIN_OUTSIDE             whether output pixel (x, y) is no pixel (default: x >= w || y >= h)
// The defaults leave the statements below what they were.
//
// The window form: the plain chain with the 21 dependent taps of v (and u, and the rates) served from LDS and lean index
// arithmetic.  Measured (round 5, profiles/r05_notes.md): the plain loop costs 4.0 us per iteration and 1080p frame at
// TWO limits at once -- the texture path takes ~19 cycles per 64-lane 8-byte gather and CU (4 gathers per tap), and its
// ~56 VALU instructions per tap (two of them quarter-rate multiplies, 64-bit address arithmetic per texel) cost the same
// in issue slots: an LDS window alone (112 us) or lean indices alone (97 us) leave the 98 us where they were, both
// together give 64 us.  A workgroup of RW x RH = 32 x 16 pixels stages one window of the field around where its pixels
// land -- the block displaced by the warp of its centre, RR cells of margin for the variation of the warp across the
// block and the path of the fixed-point iteration -- with CLAMPED source coordinates, so that window cell
// (i - ox, j - oy) holds exactly the texel tap2 fetches for the raw floor index i (tap2's clamps of i0, i0 + 1 to the
// image commute with the staging), and a tap inside the window needs no clamp at all: floor, convert, two unsigned
// compares, one multiply-add, four ds_read_b64.  A tap outside takes global gathers with the lean indices above.  Same
// float expressions in the same order: byte-identical output (tests/test_gpu_parity.py::test_render_*).  Tiles are dealt
// to the XCDs in contiguous bands (a workgroup's id modulo 8 is its XCD); the grid is ((ntiles + 7) / 8) * 8 workgroups
// of RW x RH threads.  RATES: (G, K) is staged like v in a third window, g of the last tap steers the next round, the
// four K texels and fractions of the last tap are kept and k is formed once, after round 20.
#ifndef VM_CHAIN_WIN_NO_PIXEL
#define VM_CHAIN_WIN_NO_PIXEL return
#endif
#ifndef VM_CHAIN_WIN_STAGE
#define VM_CHAIN_WIN_STAGE(ox, oy) true
#endif
#ifndef VM_CHAIN_WIN_STAGE_FIELD
#define VM_CHAIN_WIN_STAGE_FIELD true
#endif
#ifndef VM_CHAIN_WIN_Q_X
#define VM_CHAIN_WIN_Q_X (float)x
#define VM_CHAIN_WIN_Q_Y (float)y
#endif
#ifndef VM_CHAIN_WIN_ORIGIN_X
#define VM_CHAIN_WIN_ORIGIN_X bx
#define VM_CHAIN_WIN_ORIGIN_Y by
#define VM_CHAIN_WIN_CENTRE_X min(bx + RW / 2, wm1)
#define VM_CHAIN_WIN_CENTRE_Y min(by + RH / 2, hm1)
#endif
#ifndef VM_CHAIN_WIN_OUTSIDE
#define VM_CHAIN_WIN_OUTSIDE x >= w || y >= h
#endif
    int x, y;
    Landing L;
    {
        __shared__ float2 win_v[WH * WW];
        __shared__ float2 win_u[HAS_U ? WH * WW : 1];
        __shared__ float2 win_r[RATES ? WH * WW : 1];      // (G, K) per cell
        const int blk = blockIdx.x, per = (ntiles + 7) / 8;
        const int tile = (blk % 8) * per + blk / 8;         // contiguous bands of tiles per XCD
        if (tile >= ntiles)
            return;                                 // the whole workgroup
        const int bx = (tile % tiles_x) * RW, by = (tile / tiles_x) * RH;
        const int tid = threadIdx.y * RW + threadIdx.x;
        const float fw = (float)w, fh = (float)h;
        const int wm1 = w - 1, hm1 = h - 1;
        const float alpha = 0.8f;
        float s1 = 2 * geo_fa - 1;
        float s2 = 4 * geo_fa - 4 * geo_fa * geo_fa;
        int ox, oy;
        {
            const int cx = VM_CHAIN_WIN_CENTRE_X, cy = VM_CHAIN_WIN_CENTRE_Y;
            const float2 vc = vf[cy * rs + cx];
            const float2 uc = HAS_U ? uf[cy * rs + cx] : make_float2(0.0f, 0.0f);
            if constexpr (RATES) {             // the window goes where the centre's own rate sends it
                const float gc = rate_at(rates, (uint32_t)(cy * rs + cx) << 3).x;
                s1 = 2 * gc - 1;
                s2 = 4 * gc - 4 * gc * gc;
            }
            // (a non-finite or absurd centre puts the window nowhere useful: every tap then takes the global path)
            const float dx = __builtin_amdgcn_fmed3f(s1 * vc.x + s2 * uc.x, -1e6f, 1e6f), dy = __builtin_amdgcn_fmed3f(s1 * vc.y + s2 * uc.y, -1e6f, 1e6f);
            ox = VM_CHAIN_WIN_ORIGIN_X - (int)rintf(dx) - RR;
            oy = VM_CHAIN_WIN_ORIGIN_Y - (int)rintf(dy) - RR;
        }
        // staged with CLAMPED source coordinates: every index below is within the field
        if (VM_CHAIN_WIN_STAGE(ox, oy)) {
            for (int i = tid; i < WH * WW; i += RW * RH) {
                const int wy = i / WW, wx = i - wy * WW;
                const int src = min(max(oy + wy, 0), hm1) * rs + min(max(ox + wx, 0), wm1);
                if (VM_CHAIN_WIN_STAGE_FIELD) {
                    win_v[i] = vf[src];
                    if (HAS_U)
                        win_u[i] = uf[src];
                }
                if constexpr (RATES)
                    win_r[i] = rate_at(rates, (uint32_t)src << 3);
            }
            __syncthreads();
        }
        x = bx + threadIdx.x; y = by + threadIdx.y;
        if (VM_CHAIN_WIN_OUTSIDE)
            VM_CHAIN_WIN_NO_PIXEL;
        const float qx = VM_CHAIN_WIN_Q_X, qy = VM_CHAIN_WIN_Q_Y;
        float px = qx, py = qy, lx = qx, ly = qy;
        float2 v, u = make_float2(0.0f, 0.0f);
        const LdsWords wv = (LdsWords)win_v, wu = (LdsWords)win_u, wr = (LdsWords)win_r;
        // RATES: g of the last tap, and its four K texels and fractions (k is wanted after round 20 only)
        float g = 0.0f, ka = 0.0f, kb = 0.0f, k00 = 0.0f, k10 = 0.0f, k01 = 0.0f, k11 = 0.0f;
        // one tap of v (and u, and the rates) at (px + 0.5, py + 0.5): tap2's expression
        auto tap = [&](float2 &tv, float2 &tu) {
            const float xb = (px + 0.5f) - 0.5f, yb = (py + 0.5f) - 0.5f;
            const float fi = floorf(xb), fj = floorf(yb);
            const float a = xb - fi, b = yb - fj;
            const uint32_t a0 = (uint32_t)(int)fi - (uint32_t)ox, b0 = (uint32_t)(int)fj - (uint32_t)oy;
            // the window is read unconditionally (cell 0 for a tap outside), the global gathers only by the lanes outside:
            // written as "if (inside) LDS else global" the compiler merges the two into flat loads through selected pointers
            const bool inside = a0 < (uint32_t)(WW - 1) && b0 < (uint32_t)(WH - 1);
            const uint32_t c = inside ? __umul24(b0, (uint32_t)WW) + a0 : 0u;     // (24-bit multiply-add: full rate)
            // (and as volatile 8-byte words: plain loads are sunk below the branch and merged all the same)
            float2 t00 = lds8(wv, c), t10 = lds8(wv, c + 1), t01 = lds8(wv, c + WW), t11 = lds8(wv, c + WW + 1);
            float2 u00, u10, u01, u11;
            if (HAS_U) { u00 = lds8(wu, c); u10 = lds8(wu, c + 1); u01 = lds8(wu, c + WW); u11 = lds8(wu, c + WW + 1); }
            float2 r00, r10, r01, r11;
            if constexpr (RATES) { r00 = lds8(wr, c); r10 = lds8(wr, c + 1); r01 = lds8(wr, c + WW); r11 = lds8(wr, c + WW + 1); }
            if (!inside) {
                const TapIdx t = tap_index<3>(px + 0.5f, py + 0.5f, fw, fh, wm1, hm1, (uint32_t)rs);
                const char *bv = (const char *)vf, *bu = (const char *)uf;
                t00 = *(const float2 *)(bv + t.o00); t10 = *(const float2 *)(bv + t.o10);
                t01 = *(const float2 *)(bv + t.o01); t11 = *(const float2 *)(bv + t.o11);
                if (HAS_U) {
                    u00 = *(const float2 *)(bu + t.o00); u10 = *(const float2 *)(bu + t.o10);
                    u01 = *(const float2 *)(bu + t.o01); u11 = *(const float2 *)(bu + t.o11);
                }
                if constexpr (RATES) {
                    r00 = rate_at(rates, t.o00); r10 = rate_at(rates, t.o10);
                    r01 = rate_at(rates, t.o01); r11 = rate_at(rates, t.o11);
                }
            }
            tv.x = (1 - a) * (1 - b) * t00.x + a * (1 - b) * t10.x + (1 - a) * b * t01.x + a * b * t11.x;
            tv.y = (1 - a) * (1 - b) * t00.y + a * (1 - b) * t10.y + (1 - a) * b * t01.y + a * b * t11.y;
            if (HAS_U) {
                tu.x = (1 - a) * (1 - b) * u00.x + a * (1 - b) * u10.x + (1 - a) * b * u01.x + a * b * u11.x;
                tu.y = (1 - a) * (1 - b) * u00.y + a * (1 - b) * u10.y + (1 - a) * b * u01.y + a * b * u11.y;
            }
            if constexpr (RATES) {
                g = lerp2(r00.x, r10.x, r01.x, r11.x, a, b);
                ka = a; kb = b;
                k00 = r00.y; k10 = r10.y; k01 = r01.y; k11 = r11.y;
            }
        };
        {
            float2 tv, tu;
            tap(tv, tu);
            v = tv;
            if (HAS_U) u = tu;
        }
        for (int i = 0; i < VM_RENDER_ITERS; ++i) {
            lx = px; ly = py;
            if constexpr (RATES) {
                s1 = 2 * g - 1;
                s2 = 4 * g - 4 * g * g;
            }
            // (without a path u stays +0 and s2 * u is a loop invariant -- +-0, or NaN for a non-finite geo_fa: still
            // subtracted, so that the result is the plain form's in every case)
            px = qx - s1 * v.x - s2 * u.x;
            py = qy - s1 * v.y - s2 * u.y;
            float2 tv, tu;
            tap(tv, tu);
            v.x = alpha * tv.x + (1 - alpha) * v.x;
            v.y = alpha * tv.y + (1 - alpha) * v.y;
            if (HAS_U) {
                u.x = alpha * tu.x + (1 - alpha) * u.x;
                u.y = alpha * tu.y + (1 - alpha) * u.y;
            }
        }
        L.px = px; L.py = py; L.lx = lx; L.ly = ly; L.v = v; L.u = u;
        L.g = g; L.k = lerp2(k00, k10, k01, k11, ka, kb);
    }
