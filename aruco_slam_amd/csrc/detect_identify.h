// ------------------------------------------------------------------------------------------------
// k_identify body (included twice by detect.hip, see there; no include guard on purpose)
//   ASLAM_IDENT_KERNEL  the kernel's name
//   ASLAM_IDENT_RECORD  1: the kernel takes one more parameter, rec, and writes each candidate's IdentRecord to it (indexed like
//                       finals); 0: the production kernel, whose text is exactly what it was before the switch existed
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ASLAM_IDENT_KERNEL(DetectCfg cfg, Counters* ctr, const uint8_t* __restrict__ gray,
                                                 FinalCand* __restrict__ finals, const IdentWork* __restrict__ work,
                                                 const unsigned long long* __restrict__ dict_codes
#if ASLAM_IDENT_RECORD
                                                 , IdentRecord* __restrict__ rec
#endif
                                                 ) {
    __shared__ double sA[8][8];
    __shared__ double sB[8];
    __shared__ double sM[9];
    __shared__ uint8_t img[kWarpMax * kWarpMax];
    __shared__ int hist[256];
    __shared__ int sDecision[2];        // [0]: 0 = otsu, 1 = all zero bits, 2 = all one bits ; [1]: otsu threshold
    __shared__ double sOtsuA[256], sOtsuB[256], sMu;   // per bin: p_i, i p_i; then q1 (-1: skipped), mu1
    __shared__ int sOtsuRange[2];
    const int lane = threadIdx.x & 63;
    const int rows = cfg.rows, cols = cfg.cols;
    const int ms = cfg.marker_size, bb = cfg.border_bits;
    const int nc = ms + 2 * bb;                 // cells per side
    const int cell = cfg.cell_px;
    const int S = nc * cell;                    // warped image side
    const unsigned n_work = ctr->n_ident;
#ifdef ASLAM_IDENT_STAMPS
    long long ist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long ilast = clock64();
    int inum = 0;
#define IST(i) do { const long long t_ = clock64(); ist[i] += t_ - ilast; ilast = t_; } while (0)
#else
#define IST(i) do { } while (0)
#endif

    for (;;) {
        unsigned wi = 0;
        IST(7);
        if (lane == 0) wi = atomicAdd(&ctr->q_ident, 1u);
        wi = __shfl(wi, 0);
        if (wi >= n_work) break;
        const IdentWork wk = work[wi];
        FinalCand* fc = &finals[(size_t)wk.frame * kCandMax + wk.idx];
        const uint8_t* gimg = gray + (size_t)wk.frame * rows * cols;

        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        IST(0);
        {
            // cv::getPerspectiveTransform(corners -> (0,0),(S-1,0),(S-1,S-1),(0,S-1)): the 8 x 8 elimination with partial pivoting, one
            // matrix element per lane (row er = lane / 8, column ec = lane % 8; every lane of a row carries the row's right-hand side).
            // Every element goes through exactly the operations of the sequential elimination (quotient, product, difference; first
            // maximal pivot), so the result is bit-identical to it - only the 58 k cycles of dependent LDS traffic on one lane are gone.
            const int er = lane >> 3, ec = lane & 7, ei = er & 3;
            const float dstx = (ei == 1 || ei == 2) ? (float)S - 1 : 0.f;
            const float dsty = ei >= 2 ? (float)S - 1 : 0.f;
            const float sx = fc->c[2 * ei], sy = fc->c[2 * ei + 1];
            const float dst = er < 4 ? dstx : dsty;
            double ea;
            if (ec == 6) ea = -(double)sx * dst;
            else if (ec == 7) ea = -(double)sy * dst;
            else {
                const int k = er < 4 ? ec : ec - 3;                  // rows 0..3: (sx, sy, 1) in columns 0..2; rows 4..7: in columns 3..5
                ea = k == 0 ? (double)sx : k == 1 ? (double)sy : k == 2 ? 1.0 : 0.0;
            }
            double eb = dst;
            // rows are exchanged through LDS (the workgroup is one wavefront): per column one write of the matrix, then broadcast reads of
            // the pivot column, the pivot row and the right-hand side - a quarter of the LDS-pipe operations of lane-to-lane shuffles
            for (int col = 0; col < 8; col++) {
                __syncthreads();                                     // the previous column's reads are done
                sA[er][ec] = ea;
                if (ec == 0) sB[er] = eb;
                __syncthreads();
                int piv = col;
                double best = fabs(sA[col][col]);
                for (int r = col + 1; r < 8; r++) {
                    const double v = fabs(sA[r][col]);
                    if (v > best) { best = v; piv = r; }
                }
                // after the exchange row `col` holds what row `piv` held, and the other way round
                if (er == col) { ea = sA[piv][ec]; eb = sB[piv]; }
                else if (er == piv) { ea = sA[col][ec]; eb = sB[col]; }
                const double pv = sA[piv][col];
                const double mine = er == col ? pv : er == piv ? sA[col][col] : sA[er][col];
                const double rowc = sA[piv][ec], brow = sB[piv];
                if (er > col) {
                    const double fct = mine / pv;
                    if (ec >= col) ea -= fct * rowc;
                    eb -= fct * brow;
                }
            }
            __syncthreads();
            sA[er][ec] = ea;
            if (ec == 0) sB[er] = eb;
        }
        __syncthreads();
        IST(1);
        if (lane == 0) {
            double x[8];
            for (int i = 7; i >= 0; i--) {
                double s = sB[i];
                for (int c = i + 1; c < 8; c++) s -= sA[i][c] * x[c];
                x[i] = s / sA[i][i];
            }
            // cv::invert (3x3 cofactor form) for warpPerspective without WARP_INVERSE_MAP
            double m0 = x[0], m1 = x[1], m2 = x[2], m3 = x[3], m4 = x[4], m5 = x[5], m6 = x[6], m7 = x[7], m8 = 1.0;
            double det = m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
            if (det != 0.) {
                double d = 1. / det;
                sM[0] = (m4 * m8 - m5 * m7) * d;
                sM[1] = (m2 * m7 - m1 * m8) * d;
                sM[2] = (m1 * m5 - m2 * m4) * d;
                sM[3] = (m5 * m6 - m3 * m8) * d;
                sM[4] = (m0 * m8 - m2 * m6) * d;
                sM[5] = (m2 * m3 - m0 * m5) * d;
                sM[6] = (m3 * m7 - m4 * m6) * d;
                sM[7] = (m1 * m6 - m0 * m7) * d;
                sM[8] = (m0 * m4 - m1 * m3) * d;
            } else {
                for (int i = 0; i < 9; i++) sM[i] = 0;
            }
        }
        __syncthreads();

        IST(2);
        // warpPerspective(INTER_NEAREST), histogram, inner-region moments
        const int lo = cell / 2, hi = S - cell / 2;
        long long sum = 0, sq = 0;
        // (kWarpUnroll pixels per round: their gray loads are issued together, at clamped addresses - a guarded load is a branch with
        //  its own wait, and the loads of a lane's ~50 pixels would queue up behind each other)
        // pixel p = lane + 64 k of the warped image; (x, y) advanced without divisions, once for the addresses and once for the use
        const int step_y = 64 / S, step_x = 64 - step_y * S;
        int py = lane / S, px = lane - py * S;
        int qy = py, qx = px;
        for (int p0 = lane; p0 < S * S; p0 += 64 * kWarpUnroll) {
            int vv[kWarpUnroll];                                    // gray value, -1 outside the frame
#pragma unroll
            for (int u = 0; u < kWarpUnroll; u++) {
                const int x = px, y = min(py, S - 1);                // (beyond the image: any valid pixel, the value is not used)
                px += step_x; py += step_y;
                if (px >= S) { px -= S; py++; }
                double X0 = sM[1] * y + sM[2], Y0 = sM[4] * y + sM[5], W0 = sM[7] * y + sM[8];
                double W = W0 + sM[6] * x;
                W = W ? 1. / W : 0;
                double fX = fmax((double)INT_MIN, fmin((double)INT_MAX, (X0 + sM[0] * x) * W));
                double fY = fmax((double)INT_MIN, fmin((double)INT_MAX, (Y0 + sM[3] * x) * W));
                const int X = (int)rint(fX), Y = (int)rint(fY);      // clamped to the int range above: the 32-bit conversion is exact
                const bool inside = X >= 0 && X < cols && Y >= 0 && Y < rows;
                const int g = gimg[inside ? (size_t)Y * cols + X : (size_t)0];
                vv[u] = inside ? g : -1;
            }
#pragma unroll
            for (int u = 0; u < kWarpUnroll; u++) {
                const int p = p0 + 64 * u;
                const int x = qx, y = qy;
                qx += step_x; qy += step_y;
                if (qx >= S) { qx -= S; qy++; }
                if (p < S * S) {
                    const int v = max(vv[u], 0);
                    img[p] = (uint8_t)v;
                    atomicAdd(&hist[v], 1);
                    if (x >= lo && x < hi && y >= lo && y < hi) { sum += v; sq += v * v; }
                }
            }
        }
        IST(3);
        for (int o = 32; o > 0; o >>= 1) { sum += __shfl_down(sum, o); sq += __shfl_down(sq, o); }
        __syncthreads();
        // getThreshVal_Otsu_8u over the whole warped image.  Only (q1, mu1) are carried from bin to bin: one lane runs that recurrence
        // - every operation of the sequential loop, bins before the first and after the last occupied one leave nothing behind - and all
        // lanes then evaluate sigma for their bins from the stored (q1, mu1); first maximum as in the scan.
        {
            const int N = S * S;
            const double sc = 1. / N;
            long long isum = 0;                                     // sum of i * hist[i]: integers, exact in any order
            unsigned long long occupied[4];
            for (int k = 0; k < 4; k++) {
                const int i = lane + 64 * k;
                const int h = hist[i];
                const double p_i = h * sc;
                sOtsuA[i] = p_i;
                sOtsuB[i] = i * p_i;
                isum += (long long)i * h;
                occupied[k] = __ballot(h != 0);
            }
            for (int o = 32; o > 0; o >>= 1) isum += __shfl_down(isum, o);
            __syncthreads();
            if (lane == 0) {
                const double scale = 1.0 / ((double)(hi - lo) * (hi - lo));
                const double mean = sum * scale;
                const double var = fmax(sq * scale - mean * mean, 0.);
                const double stddev = sqrt(var);
                if (stddev < cfg.min_otsu_std) {
                    sDecision[0] = mean > 127 ? 2 : 1;
                    sDecision[1] = 0;
                } else {
                    sDecision[0] = 0;
                    int first = 256, last = -1;
                    for (int k = 0; k < 4; k++)
                        if (occupied[k]) { first = min(first, 64 * k + __ffsll((long long)occupied[k]) - 1); last = 64 * k + 63 - __clzll((long long)occupied[k]); }
                    sOtsuRange[0] = first; sOtsuRange[1] = last;
                    sMu = (double)isum * sc;
                    double mu1 = 0, q1 = 0;
                    for (int i = first; i <= last; i++) {
                        const double p_i = sOtsuA[i], ip_i = sOtsuB[i];
                        mu1 *= q1;
                        q1 += p_i;
                        const double q2 = 1. - q1;
                        if (fmin(q1, q2) < FLT_EPSILON || fmax(q1, q2) > 1. - FLT_EPSILON) {
                            sOtsuA[i] = -1.;                         // no sigma for this bin
                        } else {
                            mu1 = (mu1 + ip_i) / q1;
                            sOtsuA[i] = q1;
                            sOtsuB[i] = mu1;
                        }
                    }
                }
            }
            __syncthreads();
            if (sDecision[0] == 0) {                                 // uniform
                const int first = sOtsuRange[0], last = sOtsuRange[1];
                const double mu = sMu;
                double best = 0.0;
                int besti = 0x7fffffff;
                for (int k = 0; k < 4; k++) {
                    const int i = lane + 64 * k;
                    if (i >= first && i <= last) {
                        const double q1 = sOtsuA[i], mu1 = sOtsuB[i];
                        if (q1 >= 0.) {
                            const double q2 = 1. - q1;
                            const double mu2 = (mu - q1 * mu1) / q2;
                            const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
                            if (sigma > best) { best = sigma; besti = i; }
                        }
                    }
                }
                wave_first_max(best, besti);
                if (lane == 0) sDecision[1] = best > 0.0 ? besti : 0;
            }
        }
        __syncthreads();
        IST(4);
        // cell votes: up to 81 cells, lanes take cells lane and lane + 64
        unsigned long long bitsLo = 0, bitsHi = 0;       // cell index c -> bit c (lo) / c - 64 (hi)
        {
            const int dec = sDecision[0], T = sDecision[1];
            const int wcell = cell - 2 * cfg.cell_margin;
            for (int half = 0; half < 2; half++) {
                int c = lane + 64 * half;
                int bit = 0;
                if (c < nc * nc) {
                    if (dec == 2) bit = 1;
                    else if (dec == 0) {
                        int cy = c / nc, cx = c - cy * nc;
                        int Xs = cx * cell + cfg.cell_margin, Ys = cy * cell + cfg.cell_margin;
                        int nz = 0;
                        for (int yy = 0; yy < wcell; yy++)
                            for (int xx = 0; xx < wcell; xx++) nz += img[(Ys + yy) * S + Xs + xx] > T;
                        bit = nz > (wcell * wcell) / 2;
                    }
                }
                unsigned long long bm = __ballot(bit);
                if (half == 0) bitsLo = bm; else bitsHi = bm;
            }
        }
        auto cell = [&](int cy, int cx) -> int {
            int c = cy * nc + cx;
            return c < 64 ? (int)((bitsLo >> c) & 1ull) : (int)((bitsHi >> (c - 64)) & 1ull);
        };
        IST(5);
        // _getBorderErrors
        int borderErr = 0;
        for (int y = 0; y < nc; y++)
            for (int k = 0; k < bb; k++) { borderErr += cell(y, k); borderErr += cell(y, nc - 1 - k); }
        for (int x = bb; x < nc - bb; x++)
            for (int k = 0; k < bb; k++) { borderErr += cell(k, x); borderErr += cell(nc - 1 - k, x); }
        int id = -1, rot = 0;
        if (borderErr <= cfg.max_border_err) {
            // inner bits, row-major MSB first (rotation 0 of Dictionary::getByteListFromBits)
            unsigned long long code = 0;
            for (int r = 0; r < ms; r++)
                for (int c = 0; c < ms; c++) code = (code << 1) | (unsigned long long)cell(r + bb, c + bb);
            // Dictionary::identify: first marker whose best rotation is within the correction budget
            int bestM = INT_MAX, bestR = 0;
            for (int m = lane; m < cfg.n_dict; m += 64) {
                int minD = ms * ms + 1, minR = -1;
                for (int r = 0; r < 4; r++) {
                    int h = __popcll(dict_codes[(size_t)m * 4 + r] ^ code);
                    if (h < minD) { minD = h; minR = r; }
                }
                if (minD <= cfg.max_corr && m < bestM) { bestM = m; bestR = minR; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                int om = __shfl_down(bestM, o), orr = __shfl_down(bestR, o);
                if (om < bestM) { bestM = om; bestR = orr; }
            }
            bestM = __shfl(bestM, 0);
            bestR = __shfl(bestR, 0);
            if (bestM != INT_MAX) { id = bestM; rot = bestR; }
        } else {
            // keep the wave convergent: the shuffles above are executed by all lanes or by none
        }
        if (lane == 0) {
            fc->pad[0] = rot;        // corner rotation is applied when the marker list is built (k_pose)
            fc->id = id;
#if ASLAM_IDENT_RECORD
            IdentRecord& ir = rec[(size_t)wk.frame * kCandMax + wk.idx];
            ir.bits[0] = bitsLo;
            ir.bits[1] = bitsHi;
            ir.sum = sum;
            ir.sq = sq;
            ir.id = id;
            ir.rot = rot;
            ir.branch = sDecision[0];
            ir.T = sDecision[1];
            ir.border_err = borderErr;
#endif
        }
        __syncthreads();
        IST(6);
#ifdef ASLAM_IDENT_STAMPS
        inum++;
#endif
    }
#ifdef ASLAM_IDENT_STAMPS
    if (lane == 0 && blockIdx.x < 3 && n_work > 1000)
        printf("identify wave %d: %d candidates; cycles: fetch %lld, elimination %lld, back-substitution %lld, warp %lld, moments+otsu %lld, votes %lld, border+dictionary %lld, ticket %lld\n",
               (int)blockIdx.x, inum, ist[0], ist[1], ist[2], ist[3], ist[4], ist[5], ist[6], ist[7]);
#endif
}
#undef IST
