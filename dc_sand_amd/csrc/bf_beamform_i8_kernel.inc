// bf_beamform_i8_kernel.inc -- the int8 matrix-core beamformer's kernel: one template, included once by bf_beamform_mfma.hip,
// which instantiates it for every output the product has (launch_i8 there).  FORM is the way the samples reach the matrix
// cores (kStaged, kDirect, kSplit, kChain), FULL says that nr_stations is a multiple of 64 (no antenna masks), NW is the
// number of waves of a workgroup; the four switches below choose what is computed and written.  Each switch that needs an
// argument of its own brings it as a further kernel parameter, in this order and only where the switch is on: w (WEIGHTED),
// qa (QUANT), ca (COMPLEX) -- the plain kernel takes (a), the weighted quantised complex one (a, w, qa, ca).  Everything a
// switch adds stands behind `if constexpr`: a kernel whose switches are off is, instruction for instruction, the kernel
// this file made before that switch existed (DESIGN.md section 5.7 has the comparison, and the warning that goes with it:
// restructuring this body, sharing an epilogue between finish and run_chain for one, moves kChain's register allocation).
// WEIGHTED (kStaged and kChain; include/dcs_beam_weights.h, DESIGN.md section 5.7): every coefficient w is made into
// w' = RN(ghat * w) before its digits are taken (ghat[a][b] beside the terms, same addressing), and the integer sums of a
// beam are scaled by RN(s_b / 8355711) instead of 1 / 8355711 -- the same one multiply.  kStaged keeps its four factors in
// registers; kChain, with no register to spare, reads them from LDS (16 floats behind the coefficients) one register
// ahead inside its recombine loop.
// QUANT (kStaged and kChain; include/dcs_beam_quant.h, DESIGN.md section 5.8): a result register's four floats -- the very
// floats the float kernel stores -- are multiplied by the beam's gain, rounded and clamped to int8 (q8_pack), which makes
// one dword per beam: 4 consecutive bytes of the int8 tensor [c][t/16][b][t%16][{re, im}].  A 4 x 4 dword transpose inside
// each quad of lanes then leaves a lane with SIXTEEN consecutive bytes of one beam (samples 8 h .. 8 h + 7 of beam
// bw + (lane >> 4) + 4 (lane & 3), h = (lane >> 2) & 1), and the wave writes its pair of blocks with one 16-byte store
// per lane: 2 x 512 contiguous bytes.  kStaged keeps its four gains in registers, kChain reads them from LDS behind the
// weighted form's factors, one register ahead.  Clipped components are counted per lane and tallied once, at the end.
// POWER (kStaged and kChain, never with QUANT; include/dcs_beam_power.h, DESIGN.md section 5.9): a result register's four
// floats -- again the very floats the float kernel stores -- become |.|^2 of its two samples and their sum; three exchanges
// inside each group of 8 lanes (power_block_sum) finish the 16-sample block's balanced pairwise sum, the same bits in all 8
// lanes.  Lane m < 4 of a group keeps register m's sum and writes that one dword: beam bw + (lane >> 4) + 4 m of its block
// of the tensor [c][t/16][b] -- 2 x 64 contiguous bytes per wave and pair of blocks.  The weighted form's factors as in
// the float kernels.
// COMPLEX (kStaged and kChain; include/dcs_beam_complex.h, DESIGN.md section 5.13): the true complex product sum_a w_a x_a
// instead of the element-wise one.  A coefficient gives NINE operands per 64 antennas instead of six: the digits of re, of
// sigma im and of -sigma im (sigma = -1
// with bf_complex_args.conj: the sign of im is flipped before fixed_word, so the conjugate costs nothing in the loop; the
// third operand is fixed_word(-sigma im), NOT the negated digits of the second -- a digit can be -128).  Per pair of blocks
// and 64 antennas 24 MFMAs into the same twelve sums: re_d with all four planes' own samples, +im_d into the im planes with
// the re samples, -im_d into the re planes with the im samples.  |sum| <= 2 * 256 * 128 * 128 = 2^23, so s2 * 256 + s3 does
// not fit an int32: the low part is fmaf((float)s2, 256.0f, (float)s3) here -- both conversions exact, one rounding of the
// same exact integer, the integer form's bits wherever that does not wrap.  A row with a non-finite coefficient in either
// component is NaN in both planes.  Weights, factors and the detecting epilogue as in the other kernels.
// COMPLEX with QUANT (include/dcs_beam_complex_quant.h, DESIGN.md section 5.14): the quantising epilogue above, unchanged,
// applied to the complex product's result registers (kChain: the gains lie behind the factors, and those behind the
// NINE-operand coefficient image and its NaN words).

template <int FORM, bool FULL, int NW = 4, bool WEIGHTED = false, bool QUANT = false, bool POWER = false, bool COMPLEX = false, class... Extra>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(i8_waves_per_eu(FORM, FULL, QUANT, COMPLEX && WEIGHTED && !FULL))))
bf_beamform_i8_kernel(const bf_bacc_args a, const Extra... extra)
{
    constexpr uint32_t NOP = COMPLEX ? 9u : 6u; // coefficient operands per 64 antennas
    static_assert(sizeof...(Extra) == (size_t)WEIGHTED + QUANT + COMPLEX && kernel_takes<bf_weights_args, Extra...> == WEIGHTED &&
                      kernel_takes<bf_quant_args, Extra...> == QUANT && kernel_takes<bf_complex_args, Extra...> == COMPLEX,
                  "the extra parameters are w, qa, ca, each exactly where its switch is on");
    const bf_weights_args &w = kernel_extra<bf_weights_args>(extra...);
    const bf_quant_args &qa = kernel_extra<bf_quant_args>(extra...);
    const bf_complex_args &ca = kernel_extra<bf_complex_args>(extra...);
    static_assert(NW == 4 || ((NW == 8 || NW == 16) && FORM == kStaged), "8- and 16-wave workgroups exist for the staged form only");
    static_assert(!WEIGHTED || FORM == kStaged || FORM == kChain, "weights exist for the product's forms only");
    static_assert(!QUANT || (NW == 4 && (FORM == kStaged || FORM == kChain)), "the quantiser exists for the product's forms only");
    static_assert(!POWER || (!QUANT && NW == 4 && (FORM == kStaged || FORM == kChain)), "the detector exists for the product's forms only");
    static_assert(!COMPLEX || (NW == 4 && (FORM == kStaged || FORM == kChain)), "the complex product exists for the product's forms only");
    constexpr bool STAGED = FORM == kStaged, SPLIT = FORM == kSplit, CHAIN = FORM == kChain;
    extern __shared__ __attribute__((aligned(16))) char staged[]; // kStaged: the sample image (+ the coefficient exchange); kSplit: the partial sums
    uint32_t bid = BACC_LOGICAL_ID(a);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bg = bid % a.n_bgroups;
    bid /= a.n_bgroups;
    const uint32_t tg = bid % a.n_tgroups;
    const uint32_t c = bid / a.n_tgroups;
    // beam tiles per workgroup, sample blocks per round (kSplit: one tile, every wave takes every block)
    const uint32_t nbt_log2 = SPLIT || CHAIN ? 0u : a.nbt_log2;
    const uint32_t nbt = 1u << nbt_log2, tpr = SPLIT ? 1u : (uint32_t)NW >> nbt_log2;
    const uint32_t bt = SPLIT ? 0u : wave & (nbt - 1u), slot = SPLIT ? 0u : wave >> nbt_log2;
    const uint32_t kc = SPLIT || CHAIN ? wave : 0u; // the 64-antenna chunk whose coefficients this wave makes (and, kSplit, contracts)
    const uint32_t lm = lane & 15u, lg = lane >> 4;
    const uint32_t bw = (bg * nbt + bt) * 16u;     // first beam of this wave's tile
    const uint32_t tt0 = tg * a.tiles_per_wg;      // first 16-sample block of the workgroup
    const uint32_t tt1 = min(tt0 + a.tiles_per_wg, a.nT16);
    const uint32_t n_blocks = tt1 > tt0 + slot ? (tt1 - tt0 - slot + tpr - 1u) / tpr : 0u; // this wave's sample blocks
    const bool idle = bw >= a.B || n_blocks == 0u; // wave-uniform (kSplit: workgroup-uniform)
    if (!STAGED && !CHAIN && idle) return;         // (no barrier behind this in the direct form; all waves alike in kSplit)
    const bool has_chunk = !(SPLIT || CHAIN) || 64u * kc < a.A; // kSplit / kChain with <= 192 antennas: the last wave(s) have no chunk of their own
    if (STAGED) { // this wave's share of the workgroup's blocks: global -> LDS, 1 KiB per instruction, same byte order
        typedef __attribute__((address_space(3))) void lds_void;
        typedef const __attribute__((address_space(1))) void glb_void;
        const uint32_t bytes = (tt1 - tt0) * a.A * 32u; // a multiple of 32
        const char *src = reinterpret_cast<const char *>(a.ant) + ((uint64_t)c * a.nT16 + tt0) * a.A * 32u;
        for (uint32_t k = wave; k * 1024u < bytes; k += (uint32_t)NW) // a piece that overhangs the end re-reads the last 16 bytes
            __builtin_amdgcn_global_load_lds((glb_void *)(src + min(k * 1024u + lane * 16u, bytes - 16u)), (lds_void *)(staged + k * 1024u),
                                             16, 0, 0);
    }

    const uint32_t fw = a.flags[0]; // (epoch << 2) | highest pair class of the table (bf_bform_terms_kernel)
    const uint32_t cls = (fw >> 2) == a.epoch ? (fw & 3u) : DCS_CLASS_FAST_LOW;
    const float fChan = (float)c;
    const float D = a.k.fDenominator, y = a.k.fRcpDenominator;
    const float inv = 1.0f / kFixScale;
    // weighted: RN(s_b * inv) of this lane's result registers (kStaged: beam bw + (lane >> 4) + 4 r; kChain: lane i < 16 of
    // wave 0 fetches beam bw + i's, for the LDS)
    float fac[4] = {inv, inv, inv, inv};
    if constexpr (WEIGHTED && STAGED) {
#pragma unroll
        for (int r = 0; r < 4; r++) fac[r] = w.gs[min(bw + (lane >> 4) + 4u * (uint32_t)r, a.B - 1u)] * inv;
    } else if constexpr (WEIGHTED && CHAIN) {
        fac[0] = w.gs[min(bw + (lane & 15u), a.B - 1u)] * inv;
    }
    // quantised: the gains of this lane's result registers (kStaged; kChain keeps them in LDS), and this lane's clipped
    // components, byte r for register r
    float kq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t n_clip = 0u;
    if constexpr (QUANT && STAGED) {
#pragma unroll
        for (int r = 0; r < 4; r++) kq[r] = qa.gains[min(bw + (lane >> 4) + 4u * (uint32_t)r, a.B - 1u)];
    }

    // ---- coefficients: lane (row lm, group lg) holds, in byte p of each of its six operands (3 digits x {re, im}),
    //      antenna 64 kc + 4 p + lg.  16 terms loads in flight together; the fast classes fully unrolled (16 copies of
    //      ~34 instructions, nothing moves), the slow class in four rolled trips.
    // kStaged, fewer than four beam tiles per workgroup: the 4 / nbt waves that own the same tile make a quarter (half)
    // of its coefficient registers each and exchange them through LDS behind the staging barrier (the slow class makes
    // everything everywhere: its rolled loop does not split)
    const bool shared_w = STAGED && a.share_off != 0u && tpr > 1u && cls != DCS_CLASS_SLOW;
    intx4 wre[3], wim[3], wng[3]; // (wng: the complex product's -sigma im)
#pragma unroll
    for (int d = 0; d < 3; d++) wre[d] = wim[d] = wng[d] = intx4{0, 0, 0, 0};
    const uint32_t conj_bit = COMPLEX && ca.conj ? 0x80000000u : 0u; // complex: the sign of im before its digits are taken
    // A coefficient that is not finite (an infinite or NaN delay value: the slow class) has no fixed-point digits; the
    // verifier's sum for that beam and plane is NaN whatever the samples are (NaN * 0 = NaN), and so it is here: the lanes
    // note it, the wave folds the notes into one bit per result row and plane, and the rows are stored as NaN.
    bool bad_re = false, bad_im = false;
    auto make_coefficients = [&]() {
        // row i of the result tile is beam 4 (i & 3) + (i >> 2): the four lane groups of a store instruction then
        // hold four CONSECUTIVE beams (512 contiguous bytes per block) instead of every fourth
        const uint32_t beam = bw + 4u * (lm & 3u) + (lm >> 2);
        const bool beam_live = beam < a.B;
        const float *tp = a.terms + 2u * (uint64_t)min(beam, a.B - 1u);
        const float *gp = WEIGHTED ? w.gn + min(beam, a.B - 1u) : nullptr; // ghat[.][beam]
        // four antennas' words -> one register of each digit plane (a 4 x 4 byte transpose; byte z = antenna z)
        auto planes = [](const uint32_t (&g)[4], uint32_t (&out)[3]) {
            const uint32_t t0 = __builtin_amdgcn_perm(g[1], g[0], 0x05010400u), t1 = __builtin_amdgcn_perm(g[1], g[0], 0x07030602u);
            const uint32_t t2 = __builtin_amdgcn_perm(g[3], g[2], 0x05010400u), t3 = __builtin_amdgcn_perm(g[3], g[2], 0x07030602u);
            out[2] = __builtin_amdgcn_perm(t2, t0, 0x05040100u); // bytes 0: d3
            out[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u); // bytes 1: d2
            out[0] = __builtin_amdgcn_perm(t3, t1, 0x05040100u); // bytes 2: d1
        };
        // antennas 64 kc + 4 (4 q + z) + lg, z = 0..3, from their terms: one register of each of the six operands
        auto four = [&](auto gen, auto track, uint32_t q, const floatx2 (&k4)[4], const float (&g4)[4], uint32_t (&nr)[3],
                        uint32_t (&ni)[3], uint32_t (&nn)[3]) {
            uint32_t gr[4], gi[4], gn[4];
#pragma unroll
            for (uint32_t z = 0; z < 4; z++) {
                float re, im;
                gen(k4[z].x, k4[z].y, re, im);
                if constexpr (WEIGHTED) re = g4[z] * re, im = g4[z] * im;
                if (decltype(track)::value) { // the slow class only: infinite or NaN delay values end here
                    bad_re |= !(fabsf(re) <= 2.0f);
                    bad_im |= !(fabsf(im) <= 2.0f);
                }
                if constexpr (COMPLEX) im = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, im) ^ conj_bit);
                gr[z] = fixed_word(re), gi[z] = fixed_word(im);
                if constexpr (COMPLEX) gn[z] = fixed_word(-im); // the digits of the negated NUMBER
            }
            planes(gr, nr), planes(gi, ni);
            if constexpr (COMPLEX) planes(gn, nn);
            if (!FULL) { // antennas beyond nr_stations: zero digits, byte by byte
                uint32_t mask = 0;
#pragma unroll
                for (uint32_t z = 0; z < 4; z++) mask |= 64u * kc + 4u * (4u * q + z) + lg < a.A ? 0xffu << (8u * z) : 0u;
#pragma unroll
                for (int d = 0; d < 3; d++) nr[d] &= mask, ni[d] &= mask;
                if constexpr (COMPLEX) {
#pragma unroll
                    for (int d = 0; d < 3; d++) nn[d] &= mask;
                }
            }
        };
        auto generate = [&](auto gen, auto unrolled) {
            floatx2 kp[16];
            // weighted: gw[z] = ghat of antenna z, at the terms' index.  The fast classes load one group of four antennas
            // ahead (terms and ghat) instead of all sixteen terms -- what keeps kChain at 128 VGPRs and no scratch; the
            // slow class loads the ghat of its group inside its rolled loop
            float gw[16];
#pragma unroll
            for (uint32_t z = 0; z < 16; z++) {
                const uint32_t ant = 64u * kc + 4u * z + lg;
                if constexpr (WEIGHTED) {
                    if (decltype(unrolled)::value && z >= 4u) continue; // the fast classes: the others one group ahead, below
                    gw[z] = gp[(uint64_t)min(ant, a.A - 1u) * a.B];
                }
                kp[z] = *reinterpret_cast<const floatx2 *>(tp + 2u * (uint64_t)min(ant, a.A - 1u) * a.B);
            }
            if (decltype(unrolled)::value) {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    if constexpr (WEIGHTED) {
                        if (q < 3u) {
#pragma unroll
                            for (uint32_t z = 4u * q + 4u; z < 4u * q + 8u; z++) {
                                const uint32_t ant = 64u * kc + 4u * z + lg;
                                gw[z] = gp[(uint64_t)min(ant, a.A - 1u) * a.B];
                                kp[z] = *reinterpret_cast<const floatx2 *>(tp + 2u * (uint64_t)min(ant, a.A - 1u) * a.B);
                            }
                        }
                    }
                    if (shared_w && (q & (tpr - 1u)) != slot) continue; // a wave sharing its tile makes its own registers only
                    const floatx2 k4[4] = {kp[4 * q], kp[4 * q + 1], kp[4 * q + 2], kp[4 * q + 3]};
                    float g4[4] = {};
                    if constexpr (WEIGHTED) g4[0] = gw[4 * q], g4[1] = gw[4 * q + 1], g4[2] = gw[4 * q + 2], g4[3] = gw[4 * q + 3];
                    uint32_t nr[3], ni[3], nn[3];
                    four(gen, std::false_type{}, q, k4, g4, nr, ni, nn);
                    if constexpr (CHAIN) { // straight to the LDS image (component q of the chunk's six operands): the 24 registers are never held
                        uint32_t *cw = reinterpret_cast<uint32_t *>(staged) + (kc * NOP * 64u + lane) * 4u + q;
#pragma unroll
                        for (int d = 0; d < 3; d++) cw[(uint32_t)d * 256u] = beam_live ? nr[d] : 0u, cw[(3u + (uint32_t)d) * 256u] = beam_live ? ni[d] : 0u;
                        if constexpr (COMPLEX) {
#pragma unroll
                            for (int d = 0; d < 3; d++) cw[(6u + (uint32_t)d) * 256u] = beam_live ? nn[d] : 0u;
                        }
                    } else {
#pragma unroll
                        for (int d = 0; d < 3; d++) wre[d][q] = (int)nr[d], wim[d][q] = (int)ni[d];
                        if constexpr (COMPLEX) {
#pragma unroll
                            for (int d = 0; d < 3; d++) wng[d][q] = (int)nn[d];
                        }
                    }
                }
            } else { // the new register enters at the top while the others, and the loaded terms, move down -- no
                     // register is indexed by a loop variable
#pragma unroll 1
                for (uint32_t q = 0; q < 4; q++) {
                    const floatx2 k4[4] = {kp[0], kp[1], kp[2], kp[3]};
                    float g4[4] = {};
                    if constexpr (WEIGHTED) {
#pragma unroll
                        for (uint32_t z = 0; z < 4; z++) g4[z] = gp[(uint64_t)min(64u * kc + 4u * (4u * q + z) + lg, a.A - 1u) * a.B];
                    }
                    uint32_t nr[3], ni[3], nn[3];
                    four(gen, std::true_type{}, q, k4, g4, nr, ni, nn);
                    if constexpr (CHAIN) {
                        uint32_t *cw = reinterpret_cast<uint32_t *>(staged) + (kc * NOP * 64u + lane) * 4u + q;
#pragma unroll
                        for (int d = 0; d < 3; d++) cw[(uint32_t)d * 256u] = beam_live ? nr[d] : 0u, cw[(3u + (uint32_t)d) * 256u] = beam_live ? ni[d] : 0u;
                        if constexpr (COMPLEX) {
#pragma unroll
                            for (int d = 0; d < 3; d++) cw[(6u + (uint32_t)d) * 256u] = beam_live ? nn[d] : 0u;
                        }
                    } else {
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            wre[d] = intx4{wre[d][1], wre[d][2], wre[d][3], (int)nr[d]};
                            wim[d] = intx4{wim[d][1], wim[d][2], wim[d][3], (int)ni[d]};
                            if constexpr (COMPLEX) wng[d] = intx4{wng[d][1], wng[d][2], wng[d][3], (int)nn[d]};
                        }
                    }
#pragma unroll
                    for (uint32_t z = 0; z < 12; z++) kp[z] = kp[z + 4];
                }
            }
            if (!CHAIN && !beam_live) { // beams beyond nr_beams: zero coefficients (their results are not stored either)
#pragma unroll
                for (int d = 0; d < 3; d++) wre[d] = wim[d] = wng[d] = intx4{0, 0, 0, 0};
            }
        };
        if (cls == DCS_CLASS_SLOW) {
            generate([&](float kx, float ky, float &re, float &im) { coeff_slow(kx, ky, fChan, D, re, im); }, std::false_type{});
        } else {
            dispatch_fast(a.k.uDiv3Exact != 0u, cls == DCS_CLASS_FAST_LOW, [&](auto div3, auto lowdeg) {
                generate([&](float kx, float ky, float &re, float &im) {
                    coeff_fast<decltype(div3)::value, decltype(lowdeg)::value>(kx, ky, fChan, D, y, re, im);
                }, std::true_type{});
            });
        }
    };

    // ---- sample blocks, two at a time.  Column n of the B operand is NOT "sample n of one block": a lane loads the
    //      4 bytes {re, im} x samples (2 m, 2 m + 1), m = n & 7, of block A (n < 8) or block B (n >= 8) of its pair, so
    //      one 4-byte load per antenna serves FOUR contractions -- (even samples, odd samples) x (re, im) -- whose
    //      16 columns are 8 sample pairs of block A and 8 of block B.  A 4 x 4 byte transpose (8 v_perm_b32 per 4
    //      antennas) turns 16 loaded registers into the 4 K = 64 operands; a result lane holds samples 2 m and 2 m + 1 of
    //      its 4 beams: one 16-byte store each.  Half the load and store instructions of a per-block scheme and no
    //      half-word merging (d16 loads do not keep the other half with SRAM-ECC on).
    //      Global addresses (kDirect, kSplit): a wave-uniform base (scalar registers) plus a per-lane byte offset; with
    //      whole chunks (FULL) ONE offset register and the instruction's immediate (antenna 4 p + lg is 128 p bytes
    //      further), otherwise offsets clamped to the last antenna (the coefficient digits are 0 beyond nr_stations).
    //      Two load sets are in flight per wave.  hipcc waits for ALL memory operations at the head of a loop whose
    //      loads cross the back-edge, stores included, so the order inside a trip is: wait, transpose, MFMAs, STORES,
    //      then the next trip's LOADS -- one memory latency per trip, shared by loads and stores (with the loads issued
    //      first, each trip paid the load and the store latency one after the other: 3.2 us per block and wave).
    const char *ant8 = reinterpret_cast<const char *>(a.ant);
    const uint32_t blk_bytes = a.A * 32u;            // one 16-sample block of one channel: <= 8 KiB
    const uint32_t m = lm & 7u;
    const bool second = lm >= 8u;                    // this lane's columns belong to block B of the pair
    const uint32_t last = n_blocks - 1u;
    const uint32_t voff = lg * 32u + m * 4u;
    uint32_t cur[2][16];
    // "every loaded register is needed HERE": keeps the compiler from sinking a load set into the trip that consumes it
    auto arrived = [&](uint32_t (&v)[16]) {
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
        asm volatile("" : "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
    };
    auto fetch = [&](uint32_t (&dst)[16], uint32_t blk, uint32_t kc) { // pair (blk, min(blk + 1, last)), antenna chunk kc
        const uint32_t blkA = min(blk, last), blkB = min(blk + 1u, last);
        if (STAGED) { // from the LDS image: block j of the workgroup at j * blk_bytes
            const uint32_t at = ((second ? blkB : blkA) * tpr + slot) * blk_bytes + m * 4u;
#pragma unroll
            for (uint32_t p = 0; p < 16; p++)
                dst[p] = *reinterpret_cast<const uint32_t *>(staged + at + (FULL ? lg + 4u * p : min(lg + 4u * p, a.A - 1u)) * 32u);
            return;
        }
        const char *base = ant8 + ((uint64_t)c * a.nT16 + tt0 + blkA * tpr + slot) * blk_bytes; // wave-uniform
        const uint32_t hop = second ? (blkB - blkA) * tpr * blk_bytes : 0u;
        if (FULL) {
            const char *b2 = base + 2048u * kc;
            const uint32_t vo = hop + voff;
#pragma unroll
            for (uint32_t p = 0; p < 16; p++) dst[p] = *reinterpret_cast<const uint32_t *>(b2 + vo + 128u * p);
        } else {
#pragma unroll
            for (uint32_t p = 0; p < 16; p++)
                dst[p] = *reinterpret_cast<const uint32_t *>(base + (hop + min(64u * kc + lg + 4u * p, a.A - 1u) * 32u + m * 4u));
        }
    };
    // x[0] = re of the even samples, x[1] = im even, x[2] = re odd, x[3] = im odd; byte p of each = antenna 4 p + lg
    auto transpose = [&](const uint32_t (&v)[16], intx4 (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t t0 = __builtin_amdgcn_perm(v[4 * q + 1], v[4 * q], 0x05010400u);     // {a0.b0, a1.b0, a0.b1, a1.b1}
            const uint32_t t1 = __builtin_amdgcn_perm(v[4 * q + 1], v[4 * q], 0x07030602u);     // {a0.b2, a1.b2, a0.b3, a1.b3}
            const uint32_t t2 = __builtin_amdgcn_perm(v[4 * q + 3], v[4 * q + 2], 0x05010400u);
            const uint32_t t3 = __builtin_amdgcn_perm(v[4 * q + 3], v[4 * q + 2], 0x07030602u);
            x[0][q] = (int)__builtin_amdgcn_perm(t2, t0, 0x05040100u);
            x[1][q] = (int)__builtin_amdgcn_perm(t2, t0, 0x07060302u);
            x[2][q] = (int)__builtin_amdgcn_perm(t3, t1, 0x05040100u);
            x[3][q] = (int)__builtin_amdgcn_perm(t3, t1, 0x07060302u);
        }
    };
    // One load set (64 antennas of a pair of blocks) as fp32 sums f[v], plane v = (re even, im even, re odd, im odd):
    // three integer contractions from zero per plane, each exact (|sum| <= 2^20); the two low digits are combined in
    // integers (s2 * 256 + s3 < 2^29: exact), converted (one rounding, far below the result's last place), and the
    // high digit enters with one fma.
    const intx4 zero = {0, 0, 0, 0};
    // the low part of a sum: s2 * 256 + s3 as ONE fp32 rounding of the exact integer -- in int32 where that cannot wrap, with
    // an fma of the two (exactly converted) sums in the complex product, whose |s| reaches 2^23
    auto low_part = [](int s2, int s3) { return COMPLEX ? fmaf((float)s2, 256.0f, (float)s3) : (float)(s2 * 256 + s3); };
    auto contract = [&](const intx4 (&x)[4], floatx4 (&f)[4]) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            if constexpr (COMPLEX) { // plane v's own samples with re, then the other component's with +im (im planes) / -im (re planes)
                const intx4 (&wo)[3] = (v & 1) ? wim : wng;
                intx4 s3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wre[2], x[v], zero, 0, 0, 0);
                intx4 s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wre[1], x[v], zero, 0, 0, 0);
                intx4 s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wre[0], x[v], zero, 0, 0, 0);
                s3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wo[2], x[v ^ 1], s3, 0, 0, 0);
                s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wo[1], x[v ^ 1], s2, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wo[0], x[v ^ 1], s1, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) f[v][r] = fmaf((float)s1[r], 65536.0f, low_part(s2[r], s3[r]));
                continue;
            }
            const intx4 s3 = __builtin_amdgcn_mfma_i32_16x16x64_i8((v & 1) ? wim[2] : wre[2], x[v], zero, 0, 0, 0);
            const intx4 s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8((v & 1) ? wim[1] : wre[1], x[v], zero, 0, 0, 0);
            const intx4 s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8((v & 1) ? wim[0] : wre[0], x[v], zero, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) f[v][r] = fmaf((float)s1[r], 65536.0f, low_part(s2[r], s3[r]));
        }
    };
    uint32_t nan_re = 0, nan_im = 0;     // wave-uniform: rows whose re / im plane is NaN (set once the coefficients are made)
    const float fNaN = __builtin_nanf("");
    // register r of this lane is result row 4 lg + r
    auto poison = [&](int r, floatx4 &o) { // o = {re even, im even, re odd, im odd}
        if ((nan_re >> (4u * lg + (uint32_t)r)) & 1u) o[0] = fNaN, o[2] = fNaN;
        if ((nan_im >> (4u * lg + (uint32_t)r)) & 1u) o[1] = fNaN, o[3] = fNaN;
    };
    const uint32_t bb = bw + lg;         // register r of this lane: beam bb + 4 r
    const uint32_t out_blk = a.B * 128u; // bytes per 16-sample block of one channel
    char *out8 = reinterpret_cast<char *>(a.beams);
    // where this lane's 16 bytes {re, im} x samples (2 m, 2 m + 1) of beam bb + 4 r go, pair (blk, blk + 1)
    auto out_of = [&](uint32_t blk, int r) {
        const uint32_t blkA = min(blk, last), blkB = min(blk + 1u, last);
        char *base = out8 + ((uint64_t)c * a.nT16 + tt0 + blkA * tpr + slot) * out_blk; // wave-uniform
        return reinterpret_cast<floatx4 *>(base + ((second ? (blkB - blkA) * tpr * out_blk : 0u) + bb * 128u + m * 16u + 512u * r));
    };
    auto store = [&](floatx4 *dst, const floatx4 o) {
#ifdef DCS_PROBES
        if (a.plain_stores) { // probes build only: the A/B of profiles/r02_fused.md
            *dst = o;
            return;
        }
#endif
        __builtin_nontemporal_store(o, dst); // written once, read by another kernel: do not keep it in L2
    };
    // scale and store: lane l, register r = beam bw + (l >> 4) + 4 r, samples 2 m, 2 m + 1
    auto finish = [&](auto whole, uint32_t blk, const floatx4 (&f)[4]) {
        if constexpr (POWER) { // the same floats, detected: the block sum of register m stays with lane m < 4 of each 8
            float mine = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) { // beam bb + 4 r
                const float sc = WEIGHTED ? fac[r] : inv;
                floatx4 o = {f[0][r] * sc, f[1][r] * sc, f[2][r] * sc, f[3][r] * sc};
                if (nan_re | nan_im) poison(r, o);
                const float P = power_block_sum(o);
                mine = m == (uint32_t)r ? P : mine;
            }
            const uint32_t blkA = min(blk, last), blkB = min(blk + 1u, last);
            char *base = out8 + ((uint64_t)c * a.nT16 + tt0 + blkA * tpr + slot) * (a.B * 4u); // wave-uniform
            const uint32_t hop = second ? (blkB - blkA) * tpr * (a.B * 4u) : 0u;
            const uint32_t pbeam = bb + 4u * m; // (m < 4) this lane's dword: beam pbeam of block A (lanes 0 - 7 of 16) or B
            // a pair past the end repeats the last block: not stored
            if (m < 4u && (!second || blk + 1u <= last) && (decltype(whole)::value || pbeam < a.B))
                *reinterpret_cast<float *>(base + (hop + pbeam * 4u)) = mine;
            return;
        }
        if constexpr (QUANT) { // the same floats, quantised: one dword per register, transposed, one store
            const bool pair_live = !second || blk + 1u <= last; // a pair past the end repeats the last block: neither stored nor counted twice
            uint32_t pk[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { // beam bb + 4 r
                const float sc = WEIGHTED ? fac[r] : inv;
                floatx4 o = {f[0][r] * sc, f[1][r] * sc, f[2][r] * sc, f[3][r] * sc};
                if (nan_re | nan_im) poison(r, o);
                pk[r] = q8_pack(o, kq[r], qa.clips != nullptr, pair_live && (decltype(whole)::value || bb + 4u * (uint32_t)r < a.B), r, n_clip);
            }
            const uint32_t blkA = min(blk, last), blkB = min(blk + 1u, last);
            char *base = out8 + ((uint64_t)c * a.nT16 + tt0 + blkA * tpr + slot) * (a.B * 32u); // wave-uniform
            const uint32_t hop = second ? (blkB - blkA) * tpr * (a.B * 32u) : 0u;
#ifdef DCS_Q8_DWORD_STORES // the A/B of profiles/r05_beam_quant.md: four dword stores per lane, 128-byte runs
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (pair_live && (decltype(whole)::value || bb + 4u * (uint32_t)r < a.B))
                    __builtin_nontemporal_store(pk[r], reinterpret_cast<uint32_t *>(base + (hop + (bb + 4u * (uint32_t)r) * 32u + m * 4u)));
#else
            q8_quad_transpose(pk, lane);
            const uint32_t qbeam = bb + 4u * (lane & 3u); // this lane's sixteen bytes: samples 8 h .. 8 h + 7 of beam qbeam, h = (lane >> 2) & 1
            if (pair_live && (decltype(whole)::value || qbeam < a.B))
                __builtin_nontemporal_store(intx4{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]},
                                            reinterpret_cast<intx4 *>(base + (hop + qbeam * 32u + ((lane >> 2) & 1u) * 16u)));
#endif
            return;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { // beam bb + 4 r
            const float sc = WEIGHTED ? fac[r] : inv; // beam bb + 4 r's factor
            floatx4 o = {f[0][r] * sc, f[1][r] * sc, f[2][r] * sc, f[3][r] * sc};
            if (nan_re | nan_im) poison(r, o);
            if (decltype(whole)::value || bb + 4u * r < a.B) {
                floatx4 *dst = out_of(blk, r);
#ifdef DCS_PROBES
                if (a.probe == 4u) { // same bytes, but each instruction writes ONE contiguous KiB (values land in the wrong places)
                    const uint32_t blkA = min(blk, last), blkB = min(blk + 1u, last);
                    dst = reinterpret_cast<floatx4 *>(out8 + ((uint64_t)c * a.nT16 + tt0 + blkA * tpr + slot) * out_blk +
                                                      ((r >= 2 ? (blkB - blkA) * tpr * out_blk : 0u) + bw * 128u + (r & 1) * 1024u + lane * 16u));
                }
#endif
                store(dst, o);
            }
        }
    };
    // kSplit: the partial sums of two pairs meet in LDS -- [pair h][register r][chunk][lane] x 16 bytes -- and wave w
    // adds up (in chunk order), scales and stores register r = w
    floatx4 *part = reinterpret_cast<floatx4 *>(staged);
    const uint32_t n_chunks = (a.A + 63u) / 64u;
    auto park = [&](int h, const floatx4 (&f)[4]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            floatx4 o = {f[0][r], f[1][r], f[2][r], f[3][r]};
            if (nan_re | nan_im) poison(r, o); // the chunk's NaN rows reach the sum through its partial sums
            part[((h * 4 + r) * 4 + kc) * 64u + lane] = o;
        }
    };
    auto gather = [&](auto whole, int h, uint32_t blk) {
        floatx4 o = part[((h * 4 + wave) * 4 + 0) * 64u + lane];
        for (uint32_t k = 1; k < n_chunks; k++) o = o + part[((h * 4 + wave) * 4 + k) * 64u + lane];
        o = o * inv;
        if (decltype(whole)::value || bb + 4u * wave < a.B) store(out_of(blk, (int)wave), o);
    };
    auto run = [&](auto whole) {
#ifdef DCS_PROBES
        if (!SPLIT && (a.probe == 1u || a.probe == 3u || a.probe == 4u)) { // stores only: what does the memory system make of this store pattern alone?
            floatx4 f[4];
#pragma unroll
            for (int v = 0; v < 4; v++) f[v] = floatx4{(float)wre[0][0], (float)wre[1][1], (float)wim[0][2], (float)wim[2][3]};
            for (uint32_t blk = 0; blk < n_blocks; blk += 2) finish(whole, blk, f);
            return;
        }
        if (FORM == kDirect && a.probe == 2u) { // loads and stores, no arithmetic between them
            for (uint32_t blk = 0; blk < n_blocks; blk += 4) {
                arrived(cur[0]);
                arrived(cur[1]);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    floatx4 f[4];
#pragma unroll
                    for (int v = 0; v < 4; v++)
                        f[v] = floatx4{(float)cur[h][4 * v], (float)cur[h][4 * v + 1], (float)cur[h][4 * v + 2], (float)cur[h][4 * v + 3]};
                    finish(whole, blk + 2u * h, f);
                }
                __builtin_amdgcn_sched_barrier(0);
                fetch(cur[0], blk + 4u, kc);
                fetch(cur[1], blk + 6u, kc);
            }
            return;
        }
#endif
        if (STAGED) { // operands from LDS: nothing to wait for but the LDS itself
            for (uint32_t blk = 0; blk < n_blocks; blk += 2) {
                intx4 x[4];
                floatx4 f[4];
                fetch(cur[0], blk, 0u);
                transpose(cur[0], x);
                contract(x, f);
                finish(whole, blk, f);
            }
        } else { // a trip = two pairs of sample blocks (a pair past the end repeats the last block)
            for (uint32_t blk = 0; blk < n_blocks; blk += 4) {
                if (has_chunk) {
                    arrived(cur[0]);
                    arrived(cur[1]);
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        intx4 x[4];
                        floatx4 f[4];
                        transpose(cur[h], x);
                        contract(x, f);
                        if (SPLIT)
                            park(h, f);
                        else
                            finish(whole, blk + 2u * h, f);
                    }
                }
                if (SPLIT) {
                    __syncthreads(); // every chunk's partial sums are in LDS
                    gather(whole, 0, blk);
                    gather(whole, 1, blk + 2u);
                    __syncthreads(); // ... and read, before the next trip overwrites them
                }
                __builtin_amdgcn_sched_barrier(0); // the loads stay behind the stores (see above)
                if (has_chunk) {
                    fetch(cur[0], blk + 4u, kc);
                    fetch(cur[1], blk + 6u, kc);
                }
            }
        }
    };
    // the first trip's samples (kStaged: all of them, above) travel while the coefficients are made
    if (!STAGED && !CHAIN && has_chunk) fetch(cur[0], 0, kc);
    if (CHAIN && !idle) fetch(cur[0], 0, 0u); // the first (pair, chunk) of this wave's own blocks
    __builtin_amdgcn_sched_barrier(0);
#ifdef DCS_PROBES
    if (a.probe == 3u || a.probe == 4u) { // no coefficients either: the store pattern alone
#pragma unroll
        for (int d = 0; d < 3; d++) wre[d] = wim[d] = intx4{(int)lane, d, 2, 1};
    } else
#endif
    if ((shared_w || CHAIN ? bw < a.B : !idle) && has_chunk) make_coefficients(); // (kChain: a wave without blocks still makes its chunk)
    if (cls == DCS_CLASS_SLOW) { // bit i: result row i (lanes i, i + 16, i + 32, i + 48 hold its antennas) has a non-finite coefficient
        const uint64_t br = __builtin_amdgcn_ballot_w64(bad_re), bi = __builtin_amdgcn_ballot_w64(bad_im);
        nan_re = (uint32_t)((br | (br >> 16) | (br >> 32) | (br >> 48)) & 0xffffu);
        nan_im = (uint32_t)((bi | (bi >> 16) | (bi >> 32) | (bi >> 48)) & 0xffffu);
        if constexpr (COMPLEX) nan_re = nan_im = nan_re | nan_im; // both planes depend on both components
    }
    if constexpr (STAGED) {
        uint32_t *wx = reinterpret_cast<uint32_t *>(staged + a.share_off) + bt * (4u * NOP * 64u) + lane; // [tile][q][plane][lane]
        if (shared_w && bw < a.B) {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if ((q & (tpr - 1u)) == slot) {
#pragma unroll
                    for (int d = 0; d < 3; d++) wx[(q * NOP + d) * 64u] = (uint32_t)wre[d][q], wx[(q * NOP + 3u + d) * 64u] = (uint32_t)wim[d][q];
                    if constexpr (COMPLEX) {
#pragma unroll
                        for (int d = 0; d < 3; d++) wx[(q * NOP + 6u + d) * 64u] = (uint32_t)wng[d][q];
                    }
                }
        }
        __syncthreads(); // hipcc drains the LDS-DMA (vmcnt(0)) in front of it
        if (idle) return;
        if (shared_w) {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if ((q & (tpr - 1u)) != slot) {
#pragma unroll
                    for (int d = 0; d < 3; d++) wre[d][q] = (int)wx[(q * NOP + d) * 64u], wim[d][q] = (int)wx[(q * NOP + 3u + d) * 64u];
                    if constexpr (COMPLEX) {
#pragma unroll
                        for (int d = 0; d < 3; d++) wng[d][q] = (int)wx[(q * NOP + 6u + d) * 64u];
                    }
                }
        }
    } else if constexpr (CHAIN) {
        // ---- the coefficients of this wave's chunk to LDS: [chunk][operand: re d1, d2, d3, im d1, d2, d3 (complex: and -im d1, d2, d3)][lane] x 16 bytes
        intx4 *coef = reinterpret_cast<intx4 *>(staged);
        uint32_t *nanw = reinterpret_cast<uint32_t *>(staged + 4u * NOP * 64u * 16u); // [chunk][re, im]
        // (make_coefficients has written this wave's chunk: operand o of chunk k at coef[(k * NOP + o) * 64 + lane])
        if (lane == 0u) nanw[2u * wave] = has_chunk ? nan_re : 0u, nanw[2u * wave + 1u] = has_chunk ? nan_im : 0u;
        float *facw = reinterpret_cast<float *>(nanw + 8); // weighted: [16] = RN(s_b * inv) of beam bw + i
        if constexpr (WEIGHTED) {
            if (wave == 0u && lane < 16u) facw[lane] = fac[0];
        }
        if constexpr (QUANT) { // behind the factors: [16] = the gain of beam bw + i
            if (wave == 0u && lane < 16u) facw[16u + lane] = qa.gains[min(bw + lane, a.B - 1u)];
        }
        __syncthreads(); // the kernel's only barrier
        if (idle) return;
        nan_re = nanw[0] | nanw[2] | nanw[4] | nanw[6]; // a non-finite coefficient in ANY chunk poisons the row
        nan_im = nanw[1] | nanw[3] | nanw[5] | nanw[7];
        if constexpr (COMPLEX) nan_re = nan_im = nan_re | nan_im;
        const uint32_t n_chunks = (a.A + 63u) / 64u;
        auto run_chain = [&](auto whole) {
            // a step = (pair of this wave's blocks, antenna chunk), pair-major; two sample buffers in turn: the samples of step
            // s + 1 are requested before step s is worked on (step 0 was requested before the coefficient making)
            const uint32_t n_steps = ((n_blocks + 1u) >> 1) * n_chunks;
            intx4 acc[4][3];
            uint32_t s = 0, chunk = 0, blk = 0;
            uint32_t f_s = 1u, f_chunk = 1u % n_chunks, f_blk = 2u * (1u / n_chunks); // next step to request
            auto step = [&](uint32_t (&now)[16], uint32_t (&ahead)[16]) {
                arrived(now);
                if (f_s < n_steps) fetch(ahead, f_blk, f_chunk);
                f_s++;
                if (++f_chunk == n_chunks) f_chunk = 0u, f_blk += 2u;
                intx4 x[4];
                transpose(now, x);
                if (chunk == 0u) {
#pragma unroll
                    for (int v = 0; v < 4; v++)
#pragma unroll
                        for (int d = 0; d < 3; d++) acc[v][d] = zero;
                }
                if constexpr (COMPLEX) { // one operand from LDS at a time: re_d with every plane's own samples, +im_d into the im
                                         // planes with the re samples, -im_d into the re planes with the im samples
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const intx4 w = coef[(chunk * NOP + (uint32_t)d) * 64u + lane];
#pragma unroll
                        for (int v = 0; v < 4; v++) acc[v][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w, x[v], acc[v][d], 0, 0, 0);
                    }
#pragma unroll
                    for (int half = 1; half >= 0; half--) { // operands 3 - 5 (+im: v = 1, 3), then 6 - 8 (-im: v = 0, 2)
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            const intx4 w = coef[(chunk * NOP + (half ? 3u : 6u) + (uint32_t)d) * 64u + lane];
#pragma unroll
                            for (int v = half; v < 4; v += 2) acc[v][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w, x[v ^ 1], acc[v][d], 0, 0, 0);
                        }
                    }
                } else
#pragma unroll
                for (int half = 0; half < 2; half++) { // re planes (v = 0, 2), then im planes (v = 1, 3)
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const intx4 w = coef[(chunk * 6u + 3u * (uint32_t)half + (uint32_t)d) * 64u + lane];
#pragma unroll
                        for (int v = half; v < 4; v += 2) acc[v][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w, x[v], acc[v][d], 0, 0, 0);
                    }
                }
                if constexpr (POWER) {
                    if (chunk + 1u == n_chunks) { // as the float form below, each register detected and summed as it is recombined; then one dword
                        float sc_next = WEIGHTED ? facw[lg] : inv; // beam bb + 4 r's factor, one register ahead
                        float mine = 0.0f;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float sc = sc_next;
                            if constexpr (WEIGHTED) {
                                if (r < 3) sc_next = facw[4u * (uint32_t)r + 4u + lg];
                            }
                            floatx4 o;
#pragma unroll
                            for (int v = 0; v < 4; v++) o[v] = fmaf((float)acc[v][0][r], 65536.0f, low_part(acc[v][1][r], acc[v][2][r])) * sc;
                            if (nan_re | nan_im) poison(r, o);
                            const float P = power_block_sum(o);
                            mine = m == (uint32_t)r ? P : mine;
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        const uint32_t blkB = min(blk + 1u, last); // (blk <= last)
                        char *base = out8 + ((uint64_t)c * a.nT16 + tt0 + blk * tpr + slot) * (a.B * 4u); // wave-uniform
                        const uint32_t hop = second ? (blkB - blk) * tpr * (a.B * 4u) : 0u;
                        const uint32_t pbeam = bb + 4u * m;
                        if (m < 4u && (!second || blk + 1u <= last) && (decltype(whole)::value || pbeam < a.B))
                            *reinterpret_cast<float *>(base + (hop + pbeam * 4u)) = mine;
                        chunk = 0u, blk += 2u;
                    } else {
                        chunk++;
                    }
                } else
                if constexpr (QUANT) {
                    if (chunk + 1u == n_chunks) { // as below, each register quantised to one dword as it is recombined; then one store
                        const bool pair_live = !second || blk + 1u <= last;
                        uint32_t pk[4];
                        float sc_next = WEIGHTED ? facw[lg] : inv, k_next = facw[16u + lg]; // beam bb + 4 r's factor and gain, one register ahead
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float sc = sc_next, k = k_next;
                            if (r < 3) {
                                if constexpr (WEIGHTED) sc_next = facw[4u * (uint32_t)r + 4u + lg];
                                k_next = facw[16u + 4u * (uint32_t)r + 4u + lg];
                            }
                            floatx4 o;
#pragma unroll
                            for (int v = 0; v < 4; v++) o[v] = fmaf((float)acc[v][0][r], 65536.0f, low_part(acc[v][1][r], acc[v][2][r])) * sc;
                            if (nan_re | nan_im) poison(r, o);
                            pk[r] = q8_pack(o, k, qa.clips != nullptr, pair_live && (decltype(whole)::value || bb + 4u * (uint32_t)r < a.B), r, n_clip);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        const uint32_t blkB = min(blk + 1u, last); // (blk <= last)
                        char *base = out8 + ((uint64_t)c * a.nT16 + tt0 + blk * tpr + slot) * (a.B * 32u); // wave-uniform
                        const uint32_t hop = second ? (blkB - blk) * tpr * (a.B * 32u) : 0u;
#ifdef DCS_Q8_DWORD_STORES
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (pair_live && (decltype(whole)::value || bb + 4u * (uint32_t)r < a.B))
                                __builtin_nontemporal_store(pk[r], reinterpret_cast<uint32_t *>(base + (hop + (bb + 4u * (uint32_t)r) * 32u + m * 4u)));
#else
                        q8_quad_transpose(pk, lane);
                        const uint32_t qbeam = bb + 4u * (lane & 3u);
                        if (pair_live && (decltype(whole)::value || qbeam < a.B))
                            __builtin_nontemporal_store(intx4{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]},
                                                        reinterpret_cast<intx4 *>(base + (hop + qbeam * 32u + ((lane >> 2) & 1u) * 16u)));
#endif
                        chunk = 0u, blk += 2u;
                    } else {
                        chunk++;
                    }
                } else
                if (chunk + 1u == n_chunks) { // all antennas in: digits d1 = acc[v][0], d2 = acc[v][1], d3 = acc[v][2]
                    // one result register (four beams' sixteen bytes) at a time: recombined, scaled, stored -- the sixteen floats
                    // are never all alive beside the accumulators
                    float sc_next = WEIGHTED ? facw[lg] : inv; // weighted: beam bb + 4 r's factor, read one register ahead
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float sc = sc_next;
                        if constexpr (WEIGHTED) {
                            if (r < 3) sc_next = facw[4u * (uint32_t)r + 4u + lg];
                        }
                        floatx4 o;
#pragma unroll
                        for (int v = 0; v < 4; v++) o[v] = fmaf((float)acc[v][0][r], 65536.0f, low_part(acc[v][1][r], acc[v][2][r])) * sc;
                        if (nan_re | nan_im) poison(r, o);
                        if (decltype(whole)::value || bb + 4u * (uint32_t)r < a.B) store(out_of(blk, r), o);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    chunk = 0u, blk += 2u;
                } else {
                    chunk++;
                }
                s++;
            };
            while (s < n_steps) {
                step(cur[0], cur[1]);
                if (s < n_steps) step(cur[1], cur[0]);
            }
        };
        if (bw + 16u <= a.B)
            run_chain(std::true_type{});
        else
            run_chain(std::false_type{});
        if constexpr (QUANT) {
            if (qa.clips) q8_tally(qa.clips, n_clip, bb, lm, a.B);
        }
        return;
    } else if (has_chunk) {
        fetch(cur[1], 2, kc);
    }
    if (bw + 16u <= a.B)
        run(std::true_type{});
    else
        run(std::false_type{});
    if constexpr (QUANT) {
        if (qa.clips) q8_tally(qa.clips, n_clip, bb, lm, a.B);
    }
}

