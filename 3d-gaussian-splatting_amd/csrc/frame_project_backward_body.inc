// frame_project_backward_body.inc -- the body of frame_project_backward_kernel, of its GS_FRAME_POSE_GRAD variant
// frame_project_backward_pose_kernel, of the fused step's variants frame_project_backward_adam_aux_kernel and
// frame_project_backward_adam_pose_kernel and of the pose-only frame_pose_backward_kernel (project_bwd.hip), expanded in place
// in all of them.  Expects in scope: the kernel's parameters, CDIM / PART / BLOCK / ADAM, `constexpr bool POSE`,
// `constexpr bool AUX`, `constexpr bool POSE_ONLY`, `pose_part` and `pose_part_aux`.  (Included rather than called: an
// inlined device function leaves the kernel without the flag with other register assignments than before it existed;
// expanded in place, it compiles to the same code.)
    static_assert(ADAM == 0 || PART == 0, "the fused optimizer step: everything in one kernel");
    static_assert(!POSE || (CDIM == 3 && (ADAM == 0 ? PART != 2 : PART == 0)),
                  "pose gradients: rgb colours; the geometry part, or everything in front of the fused step");
    static_assert(!AUX || ADAM != 0 || POSE_ONLY,
                  "the depth map's term is formed here only in front of the fused step or in the pose-only kernel");
    // POSE_ONLY (frame_pose_backward_kernel): the row sums and the pose terms alone -- no projection or activation backward,
    // no colour part, nothing stored per Gaussian; AUX: the depth map's row as well, as in front of the fused step
    static_assert(!POSE_ONLY || (POSE && CDIM == 3 && ADAM == 0 && PART == 1), "pose only: rgb colours, the geometry part's sums");
    static_assert(gs_row_aux_depth(3) == 10, "POSE_ONLY: the depth float of an rgb row is r2.z of the row walk below");
    // rgb rows (round 4): only rows that EXIST are fetched.  71 % of the pairs of the 2.4 M scene lie behind their
    // tile's stop point and their rows are uninitialised memory; round 3 streamed all of them through LDS and looked at
    // the flags afterwards (PMC: 916 MB of traffic against 316 MB algorithmic).  Whether the row of pair (tile, g) was
    // written follows from one number per TILE -- the key of the last list entry the forward processed there (stop_keys,
    // raster_bwd.hip: stop_key_kernel): the tile's list ascends in (depth bits, Gaussian), so the row exists iff
    // key(g) <= stop key.  Every thread first turns its rectangle into a bit mask of existing rows (stop-key loads eight
    // at a time: a loop with one dependent load per row costs a memory round trip per row -- the first version of this
    // kernel: 278 us against round 3's 175), then the wave fetches the existing rows of its 64 Gaussians together, 16 rows
    // per load instruction, and every owner adds its rows up in ascending order, as before: bitwise unchanged.
    const int64_t pid0 = (int64_t)blockIdx.x * blockDim.x + g_first, pid = pid0 + threadIdx.x;
    const bool valid = pid < n;
    // (y0 | y1 << 16, x0 | x1 << 16, depth bits, tiles touched); depth bits != 0 <=> visible (depth > near > 0).  The
    // record of a culled Gaussian is unspecified (frame_project_kernel does not write it): not read.
    const uint4 rc = valid ? rects[pid] : make_uint4(0, 0, 0, 0);
    const bool vis = rc.z != 0;
    // rgb colours: the record is not needed -- sigma(opa) and the sigma(colour)s are recomputed from the raw parameters
    // (two coalesced streams, the same instructions as project_one: the same bits) instead of gathering one 64-byte
    // line per visible Gaussian for 16 + 12 of its bytes; only the "dist" listing test needs the projected centre
    const bool need_rec = CDIM > 3 || P.cull_method == 0;
    const float4 g = (vis && need_rec) ? rec_geom[pid * GS_REC_STRIDE] : make_float4(0, 0, 0, 0);
    float gp[3] = {0, 0, 0}, gqr[4] = {0, 0, 0, 0}, gsr[3] = {0, 0, 0}, gopa = 0, gcol[3] = {0, 0, 0};
    constexpr int RW4 = gs_row_floats(CDIM) / 4;  // float4s per row
    float4 d0 = make_float4(0, 0, 0, 0), d1 = d0, d2 = d0;
    const uint64_t off = vis ? pair_offsets[pid] : 0, cnt = rc.w;
    // SH: the column sums of every Gaussian's rows, [Gaussian of the workgroup][sum] with an odd stride, the sums in the
    // COMPACT order (dx, dy, da, db, dc, dd, dopa, coefficient 0 ..): the row's padding floats (gs_frame_layout.h) are
    // neither loaded nor kept
    constexpr int RWF = 4 * RW4, RS = ((7 + CDIM + 3) / 4) * 4 + 1;
    __shared__ float s_sum[CDIM > 3 ? BLOCK / GS_PB_SH_PASSES * RS : 1];
    __shared__ uint32_t s_brow[CDIM > 3 ? BLOCK / 64 : 1][64], s_bown[CDIM > 3 ? BLOCK / 64 : 1][64];

    // the stop keys as two arrays of T words: depth bits, Gaussian index (stop_key_kernel)
    const uint32_t *stop_depth = reinterpret_cast<const uint32_t *>(stop_keys);
    const uint32_t n_tiles_pb = P.ntx * P.nty;
    const uint32_t *stop_id = stop_depth + n_tiles_pb;
    // rgb: does the row of tile t = (ix, iy) of the Gaussian (depth bits dz, index id) exist?  key(g) <= stop key(t)
    auto row_exists = [&](uint32_t t, uint32_t dz, uint32_t id, uint32_t ix, uint32_t iy, float cx, float cy) {
        if (P.cull_method == 0 && !gs_dist_listed(cx, cy, ix, iy, D)) return false;  // "dist": holes in the square
        const uint32_t sd = stop_depth[t];
        return dz < sd || (dz == sd && id <= stop_id[t]);
    };
    const uint32_t my_y0 = rc.x & 0xffff, my_x0 = rc.y & 0xffff, my_x1 = rc.y >> 16;

    // A Gaussian that covers hundreds of tiles (early in training from a sparse cloud; a scale that blew up) would
    // keep ONE thread adding its rows while 255 wait: 195 us instead of 40 us for this kernel in a 500 k-Gaussian fit.
    // Such Gaussians are summed by the whole workgroup first -- thread t takes rows t, t + 256, ... straight from
    // global memory (consecutive threads, consecutive rows), a fixed shuffle tree and a fixed wave order give the
    // total to the owning thread: deterministic -- and are skipped by the per-thread loops below.
#ifndef GS_PB_BIG
#define GS_PB_BIG 64  // rows beyond which the whole workgroup sums an rgb Gaussian (A/B switch; at most 256: the row masks)
#endif
    constexpr uint32_t BIG = GS_PB_BIG;
    constexpr int NA = 12;  // floats of an rgb row that are summed (10 in use)
    constexpr int NBIG = CDIM == 3 ? 256 : 1;  // (SH rows are summed by the whole wave anyway: below)
    __shared__ uint32_t s_nbig, s_big_owner[NBIG];
    __shared__ uint64_t s_big_off[NBIG];
    __shared__ uint32_t s_big_cnt[NBIG];
    __shared__ float s_big_part[4][CDIM == 3 ? NA : 1];
    __shared__ __attribute__((aligned(16))) float s_adam_tr[ADAM ? BLOCK * 3 : 1];  // the fused optimizer step's hand-over (below)
    (void)s_adam_tr;
    const bool big = CDIM == 3 && cnt > BIG;
    if (threadIdx.x == 0) s_nbig = 0;
    __syncthreads();
    if (big) {
        const uint32_t slot = atomicAdd(&s_nbig, 1u);
        s_big_owner[slot] = threadIdx.x;
        s_big_off[slot] = off;
        s_big_cnt[slot] = (uint32_t)cnt;
    }
    __syncthreads();
    const uint32_t nbig = CDIM == 3 ? s_nbig : 0;
    for (uint32_t b = 0; b < nbig; ++b) {
        const uint64_t boff = s_big_off[b];
        const uint32_t bcnt = s_big_cnt[b];
        // the owner's rectangle and key (read back from its rectangle record: uniform over the workgroup)
        const int64_t bpid = pid0 + s_big_owner[b];
        const uint4 brc = rects[bpid];
        const uint32_t by0 = brc.x & 0xffff, bx0 = brc.y & 0xffff, bw = (brc.y >> 16) - (brc.y & 0xffff);
        float bcx = 0.f, bcy = 0.f;
        if (P.cull_method == 0) {
            const float4 bg = rec_geom[bpid * GS_REC_STRIDE];
            bcx = bg.x;
            bcy = bg.y;
        }
        float acc[NA];
#pragma unroll
        for (int e = 0; e < NA; ++e) acc[e] = 0.f;
        for (uint32_t k = threadIdx.x; k < bcnt && boff + k < max_pairs; k += 256) {
            const uint32_t iy = by0 + k / bw, ix = bx0 + k % bw;
            if (!row_exists(iy * P.ntx + ix, brc.z, (uint32_t)bpid, ix, iy, bcx, bcy)) continue;
            const float4 *row = rows + (boff + k) * RW4;
#pragma unroll
            for (int m = 0; m < NA / 4; ++m) {
                const float4 r = row[m];
                acc[4 * m] += r.x; acc[4 * m + 1] += r.y; acc[4 * m + 2] += r.z; acc[4 * m + 3] += r.w;
            }
        }
#pragma unroll
        for (int e = 0; e < NA; ++e) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[e] += __shfl_xor(acc[e], o, 64);
            if ((threadIdx.x & 63) == 0) s_big_part[threadIdx.x >> 6][e] = acc[e];
        }
        __syncthreads();
        if (threadIdx.x == s_big_owner[b]) {
            auto tot = [&](int e) {
                return (s_big_part[0][e] + s_big_part[1][e]) + (s_big_part[2][e] + s_big_part[3][e]);
            };
            d0 = make_float4(tot(0), tot(1), tot(2), tot(3));
            d1 = make_float4(tot(4), tot(5), tot(6), tot(7));
            d2 = make_float4(tot(8), tot(9), 0.f, 0.f);
        }
        __syncthreads();
    }
    if (CDIM == 3) {
        // ---- which of this Gaussian's (at most 256) rows exist: four 64-bit words, stop keys loaded eight at a time
        unsigned long long wmask[4] = {0ull, 0ull, 0ull, 0ull};
        constexpr int WAVES = BLOCK / 64;
        __shared__ uint32_t s_list[WAVES][64];   // row (relative to `rows`) of entry e of the current batch
        __shared__ float4 s_win[WAVES][64 * 3];  // the 12 leading floats of the batch's rows
        auto wave_sync = [] {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        // (Measured and dropped, round 4: looking the stop keys up wave-cooperatively as well -- the lanes list the tiles of
        // their rectangles in owner order, the wave fetches 256 stop keys in one round trip, every owner compares its own
        // -- 0.125 - 0.133 ms against 0.129 - 0.131 ms for the per-thread walk below at 2.4 M Gaussians, 0.044 against
        // 0.043 ms at cfg2: the LDS hand-overs cost what the shorter dependency chain saves.)
        if (vis && !big && cnt) {
            uint32_t ix = my_x0, iy = my_y0;  // tile of row k, advanced row by row (no division)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if ((uint32_t)w * 64u >= cnt) break;
                unsigned long long m = 0;
                for (uint32_t k0 = (uint32_t)w * 64u; k0 < (uint32_t)w * 64u + 64u && k0 < cnt; k0 += 8) {
                    uint32_t sd[8], tx8[8], ty8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool in = k0 + j < cnt;
                        tx8[j] = ix;
                        ty8[j] = iy;
                        sd[j] = in ? stop_depth[iy * P.ntx + ix] : 0u;  // 0: nothing processed / not a pair of mine
                        if (in && ++ix == my_x1) {
                            ix = my_x0;
                            ++iy;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool in = k0 + j < cnt && off + k0 + j < max_pairs;
                        bool yes = in && rc.z < sd[j];
                        // equal depth bits (the tile's stop entry itself, exact copies): the Gaussian index decides
                        if (in && rc.z == sd[j]) yes = (uint32_t)pid <= stop_id[ty8[j] * P.ntx + tx8[j]];
                        if (yes) m |= 1ull << ((k0 + j) & 63u);
                    }
                    if (P.cull_method == 0) {  // "dist": not every tile of the bounding square is listed (uniform branch)
                        for (int j = 0; j < 8; ++j)
                            if (k0 + j < cnt && !gs_dist_listed(g.x, g.y, tx8[j], ty8[j], D)) m &= ~(1ull << ((k0 + j) & 63u));
                    }
                }
                wmask[w] = m;
            }
        }
        // ---- the WAVE fetches the existing rows of its 64 Gaussians together.  A thread fetching its own rows keeps the
        // wave in the loop for as long as its busiest lane has rows (a Gaussian in front of a dense region: 9+ rows, the
        // average: 1.06), with a memory round trip per pair of rows -- 74 of the kernel's 162 us in a timing-only build
        // (profiles/r04_g_project_backward_time_split_diag.txt).  Instead the lanes' existing rows are listed in owner
        // order (LDS), the wave loads them 16 per instruction -- four lanes per aligned 64-byte line, every lane busy --
        // into an LDS window, and every owner adds ITS rows out of LDS in ascending order: the same sums, bit for bit.
        {
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
            for (int w = 0; w < 4; ++w) {  // rows 64 w .. 64 w + 63 of every Gaussian (beyond the first word: rare)
                const unsigned long long wm = wmask[w];
                if (__ballot(wm != 0ull) == 0ull) continue;  // uniform
                const uint32_t mine = (uint32_t)__popcll(wm);
                const uint32_t incl = gs_wave_incl_scan_u32(mine), first = incl - mine;
                const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                unsigned long long cm = wm;  // this lane's rows not yet added
                uint32_t done = 0;
                for (uint32_t e0 = 0; e0 < total; e0 += 64) {  // uniform trip count
                    // 1. list the entries [e0, e0 + 64) in owner order: this lane's are first + done .. first + mine - 1
                    {
                        unsigned long long lm = cm;
                        for (uint32_t e = first + done; e < e0 + 64 && lm; ++e) {
                            if (e >= e0) s_list[wv][e - e0] = (uint32_t)(off + (uint32_t)w * 64u + (uint32_t)__ffsll((long long)lm) - 1u);
                            lm &= lm - 1;
                        }
                    }
                    wave_sync();
                    // 2. the wave loads the batch: lane l = quarter l % 4 of entry 16 it + l / 4 (quarter 3 is padding)
                    const uint32_t nb = total - e0 < 64 ? total - e0 : 64u;
                    float4 v[4];
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const uint32_t j = 16u * it + ((uint32_t)lane >> 2), q = (uint32_t)lane & 3u;
                        v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (j < nb && q < 3) v[it] = rows[(size_t)s_list[wv][j] * RW4 + q];
                    }
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const uint32_t j = 16u * it + ((uint32_t)lane >> 2), q = (uint32_t)lane & 3u;
                        if (j < nb && q < 3) s_win[wv][j * 3 + q] = v[it];
                    }
                    wave_sync();
                    // 3. every owner adds its rows of this batch, ascending
                    const uint32_t lo_e = first + done > e0 ? first + done : e0;
                    const uint32_t hi_e = first + mine < e0 + 64 ? first + mine : e0 + 64;
                    for (uint32_t x = lo_e; x < hi_e; ++x) {
                        const float4 *row = &s_win[wv][(x - e0) * 3];
                        const float4 r0 = row[0], r1 = row[1], r2 = row[2];
                        d0.x += r0.x; d0.y += r0.y; d0.z += r0.z; d0.w += r0.w;
                        d1.x += r1.x; d1.y += r1.y; d1.z += r1.z; d1.w += r1.w;
                        d2.x += r2.x; d2.y += r2.y;
                        // (the depth float: the rows aux_depth_term.inc walks, in its order, from zero -- the same bits)
                        if constexpr (POSE_ONLY && AUX) d2.z += r2.z;
                        cm &= cm - 1;  // consumed
                        ++done;
                    }
                    wave_sync();  // the batch arrays are rewritten next
                }
            }
        }
    } else {
        // SH rows are 144 (224) contiguous bytes.  A thread walking its own rows issues, per row, nine (fourteen) loads
        // whose 64 lanes touch 64 different rows: the texture-address unit serialises them lane by lane -- PMC, round 2:
        // 157 such loads per wave, 0.48 ms for this kernel, with VALU and HBM both far from busy.  Instead every WAVE
        // walks the written rows of its 64 Gaussians one row per load instruction, lane c reading float c of the row
        // (one or two cache lines per instruction), and keeps the running column sums of the current Gaussian in a
        // register per lane:
        //   1. every lane (as the owner of a Gaussian) turns the one-byte flags of its next 64 rows into a bit mask --
        //      4-byte loads, four in flight;
        //   2. the set bits of all 64 owners are laid out in owner order, 64 entries (row, owner) at a time, in LDS;
        //   3. the wave takes the entries in order, eight row loads in flight; when the owner changes, the finished
        //      sums go to s_sum[owner][c] and the next owner's partial sums (zero, or what an earlier window left) come
        //      back.  A Gaussian's rows are added in ascending order from zero, exactly as its own thread did: the
        //      results are bitwise what they were, for any PART.
        // Gaussians with thousands of rows need no special path any more: the wave works through them at one row per
        // instruction.
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        // The walk runs GS_PB_SH_PASSES times, each over the rows of 64 / PASSES owners (lanes [OWN pass, OWN (pass + 1))): the
        // column sums need [OWN][RS] floats of LDS per wave instead of [64][RS] -- 30 KiB per workgroup at degree 3 left 10 of
        // the CU's 32 wave slots filled, and the walk is bound by the latency of its row loads, i.e. by how many waves wait
        // at once.  Every owner's rows are still added in ascending order from zero: bitwise the same sums.
        constexpr int OWN = 64 / GS_PB_SH_PASSES;
        float *wsum = s_sum + (size_t)wv * OWN * RS;
        // (a Gaussian beyond GS_PB_SH_BIG rows: its first row holds the total of all of them, sh_big_rows_kernel)
        const bool big_sh = cnt > (uint64_t)GS_PB_SH_BIG;
        const uint64_t nrow_all = off + cnt < max_pairs ? cnt : (max_pairs > off ? max_pairs - off : 0);
        const uint64_t nrow = big_sh ? (nrow_all ? 1 : 0) : nrow_all;
        uint32_t maxrows = (uint32_t)(nrow < 0xffffffffull ? nrow : 0xffffffffull);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t x = __shfl_xor(maxrows, o, 64);
            maxrows = x > maxrows ? x : maxrows;
        }
        const float *rowf = reinterpret_cast<const float *>(rows);
        const int cidx = lane < RWF ? gs_row_compact(CDIM, lane) : -1;  // this lane's float of a row, in the compact order
        auto wave_sync = [] {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        // Which of this lane's rows exist (at most 64: a Gaussian beyond GS_PB_SH_BIG = 64 rows presents one), once for both
        // passes: key(g) <= the stop key of the row's tile (round 5; until then a flag byte per row, written by the raster
        // backward and cleared by a memset per frame).  Stop keys eight at a time, the tile advanced row by row, as in the
        // rgb branch above.
        unsigned long long written_all = 0;
        if (big_sh) {
            written_all = nrow ? 1ull : 0ull;
        } else if (nrow) {
            const uint32_t m = nrow < 64 ? (uint32_t)nrow : 64u;  // (nrow <= GS_PB_SH_BIG = 64 here)
            uint32_t iy = my_y0, ix = my_x0;
            for (uint32_t j0 = 0; j0 < m; j0 += 8) {
                uint32_t sd[8], tx8[8], ty8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool in = j0 + j < m;
                    tx8[j] = ix;
                    ty8[j] = iy;
                    sd[j] = in ? stop_depth[iy * P.ntx + ix] : 0u;
                    if (in && ++ix == my_x1) {
                        ix = my_x0;
                        ++iy;
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool in = j0 + j < m;
                    bool yes = in && rc.z < sd[j];
                    if (in && rc.z == sd[j]) yes = (uint32_t)pid <= stop_id[ty8[j] * P.ntx + tx8[j]];
                    if (yes && P.cull_method == 0 && !gs_dist_listed(g.x, g.y, tx8[j], ty8[j], D)) yes = false;
                    if (yes) written_all |= 1ull << (j0 + j);
                }
            }
        }
        static_assert(GS_PB_SH_BIG <= 64, "one 64-bit row mask per Gaussian");
        for (int pass = 0; pass < GS_PB_SH_PASSES; ++pass) {
        const int own0 = pass * OWN;
        const bool mine_pass = lane >= own0 && lane < own0 + OWN;
        for (int i = lane; i < OWN * RS; i += 64) wsum[i] = 0.f;
        wave_sync();
        float acc = 0.f;
        int cur = -1;  // owner whose sums `acc` holds (wave-uniform)
        for (uint32_t k0 = 0; k0 < maxrows; k0 += 64) {  // windows of 64 rows per owner (uniform trip count)
            const unsigned long long written = (k0 == 0 && mine_pass) ? written_all : 0ull;
            const uint32_t mine = (uint32_t)__popcll(written);
            const uint32_t incl = gs_wave_incl_scan_u32(mine), first = incl - mine;
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            for (uint32_t e0 = 0; e0 < total; e0 += 64) {  // batches of 64 entries, in owner order (uniform)
                {
                    unsigned long long mm = written;
                    uint32_t e = first;
                    while (mm && e < e0 + 64) {
                        const uint32_t k = (uint32_t)__ffsll((long long)mm) - 1;
                        mm &= mm - 1;
                        if (e >= e0) {
                            s_brow[wv][e - e0] = (uint32_t)(off + k0 + k);  // < max_pairs < 2^30
                            s_bown[wv][e - e0] = (uint32_t)lane;
                        }
                        ++e;
                    }
                }
                wave_sync();
                const uint32_t nb = total - e0 < 64 ? total - e0 : 64u;
                constexpr uint32_t U = GS_PB_SH_U;  // row loads in flight per wave
                for (uint32_t e = 0; e < nb; e += U) {
                    float v[U];
                    uint32_t own[U];
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) {
                        const bool ok = e + u < nb;
                        const uint32_t row = __builtin_amdgcn_readfirstlane(s_brow[wv][ok ? e + u : 0]);
                        own[u] = __builtin_amdgcn_readfirstlane(s_bown[wv][ok ? e + u : 0]);
                        v[u] = (ok && cidx >= 0) ? rowf[(size_t)row * RWF + lane] : 0.f;
                    }
#pragma unroll
                    for (uint32_t u = 0; u < U; ++u) {
                        if (e + u >= nb) break;  // uniform
                        if ((int)own[u] != cur) {  // uniform
                            if (cur >= 0 && cidx >= 0) wsum[(cur - own0) * RS + cidx] = acc;
                            cur = (int)own[u];
                            acc = cidx >= 0 ? wsum[(cur - own0) * RS + cidx] : 0.f;
                        }
                        acc += v[u];
                    }
                }
                wave_sync();  // the batch arrays are rewritten next
            }
        }
        if (cur >= 0 && cidx >= 0) wsum[(cur - own0) * RS + cidx] = acc;
        wave_sync();
        if (mine_pass) {
            const float *t = wsum + (lane - own0) * RS;  // this thread's Gaussian: (dx, dy, da, db | dc, dd, dopa, coefficient 0 | ...)
            d0 = make_float4(t[0], t[1], t[2], t[3]);
            d1 = make_float4(t[4], t[5], t[6], t[7]);
        }
        if (PART != 1) {
            // coefficient gradients: CDIM consecutive floats per Gaussian in grad_rgb, the pass's OWN Gaussians -- written
            // by the wave as one contiguous run (a culled Gaussian's sums are the zeros the array started with)
            const int64_t g0w = pid0 + (int64_t)wv * 64 + own0;
            const int ng = n - g0w < OWN ? (int)(n - g0w) : OWN;  // Gaussians of this pass inside the array (may be <= 0)
            if constexpr (ADAM != 0) {
                // the fused optimizer step of the run's coefficients (round 6: SH colours too): the wave walks its contiguous
                // run of the coefficient array and of the two moments -- a kilobyte per instruction -- and applies gs_adam_one
                // with the gradients it would have stored.  Nothing else reads the raw coefficients
                // in this kernel, and a Gaussian's coefficients belong to this wave alone.
                if (!(A.skip_if_nonzero && *A.skip_if_nonzero)) {  // (uniform: an overflowed frame takes no step)
                    float *pp = A.p_rgb + g0w * CDIM, *mm = A.m_rgb + g0w * CDIM, *vv = A.v_rgb + g0w * CDIM;
                    const int ne = ng > 0 ? ng * CDIM : 0, ne4 = ne & ~3;
                    auto one = [&](float &pe, float &me, float &ve, int e) {
                        const int gl = e / CDIM, c = e - gl * CDIM;
                        gs_adam_one(pe, wsum[gl * RS + 7 + c], me, ve, A.step_rgb, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt,
                                    A.eps);
                    };
                    // float4 by float4 (the run starts at a multiple of 32 Gaussians: 16-byte aligned with the arrays) ...
                    for (int e = lane * 4; e < ne4; e += 256) {
                        typedef float nt4v __attribute__((ext_vector_type(4)));
                        float4 pv = *reinterpret_cast<const float4 *>(pp + e), mv, vw;
                        if (ADAM == 2) {
                            const nt4v a = __builtin_nontemporal_load(reinterpret_cast<const nt4v *>(mm + e));
                            const nt4v b = __builtin_nontemporal_load(reinterpret_cast<const nt4v *>(vv + e));
                            mv = make_float4(a.x, a.y, a.z, a.w), vw = make_float4(b.x, b.y, b.z, b.w);
                        } else {
                            mv = *reinterpret_cast<const float4 *>(mm + e);
                            vw = *reinterpret_cast<const float4 *>(vv + e);
                        }
                        one(pv.x, mv.x, vw.x, e);
                        one(pv.y, mv.y, vw.y, e + 1);
                        one(pv.z, mv.z, vw.z, e + 2);
                        one(pv.w, mv.w, vw.w, e + 3);
                        *reinterpret_cast<float4 *>(pp + e) = pv;
                        if (ADAM == 2) {
                            __builtin_nontemporal_store(nt4v{mv.x, mv.y, mv.z, mv.w}, reinterpret_cast<nt4v *>(mm + e));
                            __builtin_nontemporal_store(nt4v{vw.x, vw.y, vw.z, vw.w}, reinterpret_cast<nt4v *>(vv + e));
                        } else {
                            *reinterpret_cast<float4 *>(mm + e) = mv;
                            *reinterpret_cast<float4 *>(vv + e) = vw;
                        }
                    }
                    // ... and the up to three elements an array that ends inside the run leaves over
                    if (const int e = ne4 + lane; e < ne) {
                        float pe = pp[e], me = mm[e], ve = vv[e];
                        one(pe, me, ve, e);
                        pp[e] = pe, mm[e] = me, vv[e] = ve;
                    }
                }
            } else {
                float *dst = grad_rgb + g0w * CDIM;
                for (int e = lane; e < ng * CDIM; e += 64) {
                    const int gl = e / CDIM, c = e - gl * CDIM;
                    dst[e] = wsum[gl * RS + 7 + c];
                }
            }
        }
        wave_sync();  // (the next pass clears the sums)
        }
    }
    // (ADAM: the epilogue's LDS hand-over is the whole wave's, POSE: the pose sum the whole workgroup's; an invalid thread is culled: zeros)
    if (ADAM == 0 && !POSE && !valid) return;
    [[maybe_unused]] float pose[POSE ? 12 : 1];
    if constexpr (POSE) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[e] = 0.f;
    }
    // (POSE in front of the fused step, AUX frames: the depth map's pose terms, a second row per workgroup -- what
    // frame_aux_depth_pose_backward_kernel leaves behind gs_frame_backward)
    [[maybe_unused]] float pt[POSE && AUX ? 12 : 1];
    if constexpr (POSE && AUX) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pt[e] = 0.f;
    }
    if (vis && PART != 2) {
        float p[3], sraw[3], q[4], s[3];
        load3(pos, pid, p);
        load3(scale, pid, sraw);
        float4 q4 = quat[pid];
        float qraw[4] = {q4.x, q4.y, q4.z, q4.w};
        activate(qraw, sraw, P.scale_act, q, s);
        float gi[3] = {d0.x, d0.y, 0.0f}, g2[4] = {d0.z, d0.w, d1.x, d1.y};
        if constexpr (POSE_ONLY) {
            // (AUX: U[a][0] stated explicitly, as in front of the fused step -- pose_terms, project_bwd.hip)
            pose_terms<AUX>(p, q, s, P.cam, gi, g2, pose);
        } else {
        float gq[4], gs[3];
        project_backward(p, q, s, P.cam, gi, g2, gp, gq, gs);
        if constexpr (POSE) pose_terms<POSE && AUX>(p, q, s, P.cam, gi, g2, pose);
        // q_hat = q / |q|  ->  dq = (dq_hat - q_hat (q_hat . dq_hat)) / |q|
        const float inr = gs_rsq(qraw[0] * qraw[0] + qraw[1] * qraw[1] + qraw[2] * qraw[2] + qraw[3] * qraw[3]);
        float dt = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) gqr[k] = (gq[k] - q[k] * dt) * inr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (P.scale_act == 0)  // |s| + 1e-4 : d/ds = sign(s)
                gsr[k] = sraw[k] > 0 ? gs[k] : (sraw[k] < 0 ? -gs[k] : 0.0f);
            else  // trunc_exp backward (renderer.py:97-100): g * exp(clamp(x, -1, 1))
                gsr[k] = gs[k] * expf(fminf(fmaxf(sraw[k], -1.0f), 1.0f));
        }
        }
    }
    if (vis && PART != 1) {
        if (CDIM == 3) {
            // sigma(opa), sigma(colour): the expressions of project_one, which wrote them into the record
            const float so = sigmoid_f(opa_raw[pid]);
            const float c0 = sigmoid_f(rgb_raw[pid * 3 + 0]), c1 = sigmoid_f(rgb_raw[pid * 3 + 1]);
            const float c2 = sigmoid_f(rgb_raw[pid * 3 + 2]);
            gopa = d1.z * so * (1.0f - so);
            gcol[0] = d1.w * c0 * (1.0f - c0);
            gcol[1] = d2.x * c1 * (1.0f - c1);
            gcol[2] = d2.y * c2 * (1.0f - c2);
        } else {
            gopa = d1.z * g.w * (1.0f - g.w);
        }
    }
    // (POSE: both sums hold a __syncthreads -- every thread of the workgroup, the fused step's skipped frames included.  The
    // projection's row is summed here, in front of the depth map's row walk: its twelve registers are free by then)
    if constexpr (POSE) pose_block_sum<BLOCK>(pose, pose_part + (size_t)blockIdx.x * 12);
    if constexpr (AUX) {
        // GS_FRAME_AUX frames in front of the fused step (gs_frame_backward_adam_aux): what frame_aux_depth_backward_kernel adds
        // to the stored grad_pos behind this kernel is added to gp here -- the same row walk (aux_depth_term.inc), and
        // fl(gp) + gpa in that order (no contraction in this file): the step sees the bits gs_frame_backward leaves
        if (vis) {
            const float *const rows_f = reinterpret_cast<const float *>(rows);
            float ga[3];
            {
                const float *const rows = rows_f;
                // (POSE_ONLY: a Gaussian its own thread summed has g_d from that walk; one the whole workgroup summed -- a
                // tree, not this order -- walks its rows here)
                [[maybe_unused]] const bool gd_known = POSE_ONLY && !big;
                [[maybe_unused]] const float gd_sum = d2.z;
#include "aux_depth_term.inc"
#pragma unroll
                for (int c = 0; c < 3; ++c) ga[c] = gpa[c];
                if constexpr (POSE) {  // gc p^T, gc: aux_depth_backward_body.inc
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) pt[r * 3 + c] = gc[r] * p[c];
                        pt[9 + r] = gc[r];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) gp[c] = gp[c] + ga[c];
        }
    }
    if constexpr (POSE) {
        if constexpr (AUX) pose_block_sum<BLOCK, 1>(pt, pose_part_aux + (size_t)blockIdx.x * 12);
        if constexpr (ADAM == 0) {
            if (!valid) return;
        }  // (the fused step's LDS hand-over needs every lane of the wave: its invalid threads leave in the epilogue)
    }
    if constexpr (POSE_ONLY) return;  // both rows are in: nothing is stored per Gaussian
    if constexpr (ADAM != 0) {
        // ---- the optimizer step of the wave's 64 x 14 parameters (gs_adam_one: torch's _single_tensor_adam); a culled
        // Gaussian takes its zero-gradient step (momentum), as gs_adam_step gives it.  Every global access is a whole
        // float4 per lane over a contiguous run of the wave: a thread owns a GAUSSIAN, but the three [N, 3] arrays (and
        // their moments) are walked by ELEMENT -- the wave's 192 gradients go through LDS once ([Gaussian][3] in, float4
        // by float4 out, 48 lanes) and lane l updates elements 4 l .. 4 l + 3 of the wave's run.  (First version, r05_q:
        // every thread its own 14 parameters, 84 four-byte accesses at a 12-byte stride -- 0.19 ms SLOWER than
        // backward + gs_adam_step at 2.4 M Gaussians.)  The lanes that write a Gaussian's parameters are lanes of the
        // wave that read them (above, in program order): nobody else's.  (Measured and dropped, r5s: every load of the step
        // issued first -- one round trip per wave instead of five, 86 VGPRs and 9 KiB more LDS: 1,750 against 1,785 it/s
        // at 376 k Gaussians, 942 against 950 at 2.4 M; the other waves of the CU already cover the round trips.)
        if (A.skip_if_nonzero && *A.skip_if_nonzero) return;  // the frame overflowed and was rendered empty: no step (uniform)
        typedef float nt4 __attribute__((ext_vector_type(4)));
        auto ld4 = [](const float *q) {
            if (ADAM == 2) {
                const nt4 x = __builtin_nontemporal_load(reinterpret_cast<const nt4 *>(q));
                return make_float4(x.x, x.y, x.z, x.w);
            }
            return *reinterpret_cast<const float4 *>(q);
        };
        auto st4 = [](float *q, float4 x) {
            if (ADAM == 2)
                __builtin_nontemporal_store(nt4{x.x, x.y, x.z, x.w}, reinterpret_cast<nt4 *>(q));
            else
                *reinterpret_cast<float4 *>(q) = x;
        };
        auto one4 = [&](float4 &pv, float4 gv, float4 &mv, float4 &vv, float step) {
            gs_adam_one(pv.x, gv.x, mv.x, vv.x, step, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
            gs_adam_one(pv.y, gv.y, mv.y, vv.y, step, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
            gs_adam_one(pv.z, gv.z, mv.z, vv.z, step, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
            gs_adam_one(pv.w, gv.w, mv.w, vv.w, step, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
        };
        const int a_lane = threadIdx.x & 63, a_wv = threadIdx.x >> 6;
        float *tr = s_adam_tr + a_wv * 192;
        const int64_t wbase = pid0 + (int64_t)a_wv * 64, left = n - wbase;  // the wave's first Gaussian; how many lie inside
        const int ne = left >= 64 ? 192 : (left > 0 ? (int)left * 3 : 0);  // elements of the wave's run of an [N, 3] array
        const int e0 = a_lane * 4;
        auto step3 = [&](float *P3, float *M3, float *V3, const float (&g3)[3], float step, float *stat) {
            tr[a_lane * 3 + 0] = g3[0];
            tr[a_lane * 3 + 1] = g3[1];
            tr[a_lane * 3 + 2] = g3[2];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (e0 + 4 <= ne) {
                const int64_t b = wbase * 3 + e0;
                const float4 gv = *reinterpret_cast<const float4 *>(tr + e0);
                float4 pv = *reinterpret_cast<const float4 *>(P3 + b), mv = ld4(M3 + b), vv = ld4(V3 + b);
                one4(pv, gv, mv, vv, step);
                *reinterpret_cast<float4 *>(P3 + b) = pv;
                st4(M3 + b, mv);
                st4(V3 + b, vv);
                if (stat) {
                    float4 sv = *reinterpret_cast<const float4 *>(stat + b);
                    if (A.stat_mode == 1)
                        sv = make_float4(fmaxf(sv.x, fabsf(gv.x)), fmaxf(sv.y, fabsf(gv.y)), fmaxf(sv.z, fabsf(gv.z)),
                                         fmaxf(sv.w, fabsf(gv.w)));
                    else
                        sv = make_float4(sv.x + fabsf(gv.x), sv.y + fabsf(gv.y), sv.z + fabsf(gv.z), sv.w + fabsf(gv.w));
                    *reinterpret_cast<float4 *>(stat + b) = sv;
                }
            } else {
                for (int e = e0; e < ne; ++e) {  // the ragged end of the array (N not a multiple of 4): element by element
                    const int64_t b = wbase * 3 + e;
                    const float ge = tr[e];
                    float pe = P3[b], me = M3[b], ve = V3[b];
                    gs_adam_one(pe, ge, me, ve, step, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
                    P3[b] = pe;
                    M3[b] = me;
                    V3[b] = ve;
                    if (stat) stat[b] = A.stat_mode == 1 ? fmaxf(stat[b], fabsf(ge)) : stat[b] + fabsf(ge);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (the next array's gradients overwrite tr)
        };
        step3(A.p_pos, A.m_pos, A.v_pos, gp, A.step_pos, A.stat_mode ? A.stat : nullptr);
        step3(A.p_scale, A.m_scale, A.v_scale, gsr, A.step_scale, nullptr);
        if constexpr (CDIM == 3) step3(A.p_rgb, A.m_rgb, A.v_rgb, gcol, A.step_rgb, nullptr);  // (SH: stepped by the wave, above)
        if (!valid) return;
        {  // the quaternion: the thread's own float4s
            float4 pv = *reinterpret_cast<const float4 *>(A.p_quat + pid * 4), mv = ld4(A.m_quat + pid * 4);
            float4 vv = ld4(A.v_quat + pid * 4);
            one4(pv, make_float4(gqr[0], gqr[1], gqr[2], gqr[3]), mv, vv, A.step_quat);
            *reinterpret_cast<float4 *>(A.p_quat + pid * 4) = pv;
            st4(A.m_quat + pid * 4, mv);
            st4(A.v_quat + pid * 4, vv);
        }
        float po = A.p_opa[pid], mo = A.m_opa[pid], vo = A.v_opa[pid];
        gs_adam_one(po, gopa, mo, vo, A.step_opa, A.one_m_b1, A.b2, A.one_m_b2, A.inv_bc2_sqrt, A.eps);
        A.p_opa[pid] = po;
        A.m_opa[pid] = mo;
        A.v_opa[pid] = vo;
        return;
    }
    if (PART != 2) {
        grad_pos[pid * 3 + 0] = gp[0];
        grad_pos[pid * 3 + 1] = gp[1];
        grad_pos[pid * 3 + 2] = gp[2];
        grad_quat[pid] = make_float4(gqr[0], gqr[1], gqr[2], gqr[3]);
        grad_scale[pid * 3 + 0] = gsr[0];
        grad_scale[pid * 3 + 1] = gsr[1];
        grad_scale[pid * 3 + 2] = gsr[2];
    }
    if (PART == 1) return;
    grad_opa[pid] = gopa;
    if constexpr (CDIM == 3) {
        grad_rgb[pid * 3 + 0] = gcol[0];
        grad_rgb[pid * 3 + 1] = gcol[1];
        grad_rgb[pid * 3 + 2] = gcol[2];
    }  // (SH: the coefficient gradients were written by the wave, above)
