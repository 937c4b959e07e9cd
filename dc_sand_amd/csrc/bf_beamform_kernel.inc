// bf_beamform_kernel.inc -- the per-sample fused beamformer's kernel: one template, included once by bf_kernels.hip.  CH is
// the number of channels a pass takes together.  WEIGHTED applies per-input beam weights and brings its argument as a
// second kernel parameter, w; the unweighted kernel takes (a) alone and is, instruction for instruction, what it was before
// weights existed (as bf_beamform_i8_kernel's switches: DESIGN.md section 5.7).
// WEIGHTED: each coefficient w becomes w' = RN(ghat * w) (ghat[a][b] beside the terms, same addressing), the products
// and the sums are those described in bf_kernels.hip, and the beam's sums are multiplied by s_b once, at the store.
template <int CH, bool WEIGHTED = false, class... Extra>
__global__ void __launch_bounds__(kBlock) bf_beamform_kernel(const bf_beamform_args a, const Extra... extra)
{
    static_assert(sizeof...(Extra) == (size_t)WEIGHTED && kernel_takes<bf_weights_args, Extra...> == WEIGHTED,
                  "the extra parameter is w, exactly where WEIGHTED is on");
    const bf_weights_args &w = kernel_extra<bf_weights_args>(extra...);
    extern __shared__ __attribute__((aligned(16))) float s_ant[]; // [CH][A][16][2], int8 samples converted once

    const uint32_t bid = blockIdx.x;
    const uint32_t bg = bid % a.n_bgroups;
    const uint32_t rest = bid / a.n_bgroups;
    const uint32_t cb = rest % a.n_cblocks;
    const uint32_t tex = rest / a.n_cblocks; // 16-sample block within this launch

    const uint32_t b_local = threadIdx.x & 15u, t_in = threadIdx.x >> 4;
    const uint32_t b = bg * 16u + b_local;
    const uint32_t t = tex * 16u + t_in; // time index within this launch's terms table
    const bool live = b < a.B;

    // highest pair class over these 16 time steps (bf_bform_terms_kernel)
    const uint32_t fw = a.flags[tex * 16u + (threadIdx.x & 15u)];
    const uint32_t fl = (fw >> 2) == a.epoch ? (fw & 3u) : DCS_CLASS_FAST_LOW; // bf_bform_terms_kernel's epoch-tagged word
    const int slow = __syncthreads_or((int)(fl == DCS_CLASS_SLOW));
    const int high = __syncthreads_or((int)(fl != DCS_CLASS_FAST_LOW));

    const float D = a.k.fDenominator, y = a.k.fRcpDenominator;
    const float *tp = a.terms + 2u * ((uint64_t)t * a.A * a.B + (live ? b : 0u));
    const float *gp = WEIGHTED ? w.gn + (live ? b : 0u) : nullptr; // ghat[.][b]
    const uint32_t cbeg = cb * a.chan_per_block;
    const uint32_t cend = min(cbeg + a.chan_per_block, a.C);
    const uint32_t tex_g = a.tex0 + tex; // 16-sample block within the whole tensor
    const uint32_t words = a.A * 8u;     // dwords of one [A][16][2] int8 block
    const uint32_t sa = min(kAntChunk, a.A); // antennas per staged chunk = stride of a channel's LDS region

    for (uint32_t c = cbeg; c < cend; c += CH) {
        float fChan[CH], acc_re[CH], acc_im[CH];
#pragma unroll
        for (int h = 0; h < CH; h++) {
            fChan[h] = (float)(c + h);
            acc_re[h] = 0.0f;
            acc_im[h] = 0.0f;
        }
        // antennas in chunks of kAntChunk (the LDS staging buffer); the running sums carry
        // across chunks, so the summation order stays the verifier's (a = 0, 1, 2, ...)
        for (uint32_t a0 = 0; a0 < a.A; a0 += kAntChunk) {
            const uint32_t na = min(kAntChunk, a.A - a0);
            const uint32_t cw = na * 8u; // dwords of this chunk's [na][16][2] int8 block
            __syncthreads();             // previous chunk's readers are done
#pragma unroll
            for (int h = 0; h < CH; h++) {
                if (c + h < cend) {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.ant) +
                                          ((uint64_t)(c + h) * a.nt16_total + tex_g) * words + (uint64_t)a0 * 8u;
                    for (uint32_t i = threadIdx.x; i < cw; i += kBlock) {
                        const uint32_t w = src[i]; // {re, im, re, im} of two consecutive (antenna, time) samples
                        const floatx4 f = {(float)(int8_t)(w & 0xffu), (float)(int8_t)((w >> 8) & 0xffu),
                                           (float)(int8_t)((w >> 16) & 0xffu), (float)(int8_t)(w >> 24)};
                        *reinterpret_cast<floatx4 *>(&s_ant[((size_t)h * sa * 8u + i) * 4u]) = f;
                    }
                }
            }
            __syncthreads();

            auto sample = [&](int h, uint32_t al, float &sre, float &sim) {
                const floatx2 v = *reinterpret_cast<const floatx2 *>(&s_ant[(((size_t)h * sa + al) * 16u + t_in) * 2u]);
                sre = v.x;
                sim = v.y;
            };
            if (!slow) {
                dispatch_fast(a.k.uDiv3Exact != 0u, !high, [&](auto div3, auto lowdeg) {
                    // terms of antenna al+2 are requested while al is computed (L2 latency >> one step)
                    // (weighted: {rate, phase, ghat, -})
                    auto terms_of = [&](uint32_t al) {
                        if constexpr (WEIGHTED) {
                            const uint64_t i = (uint64_t)(a0 + min(al, na - 1u)) * a.B;
                            const floatx2 k = *reinterpret_cast<const floatx2 *>(tp + 2u * i);
                            return floatx4{k.x, k.y, gp[i], 0.0f};
                        } else {
                            return *reinterpret_cast<const floatx2 *>(tp + 2u * (uint64_t)(a0 + min(al, na - 1u)) * a.B);
                        }
                    };
                    auto products = [&](uint32_t al, const auto kp) {
#pragma unroll
                        for (int h = 0; h < CH; h++) {
                            float re, im, sre, sim;
                            coeff_fast<decltype(div3)::value, decltype(lowdeg)::value>(kp.x, kp.y, fChan[h], D, y, re, im);
                            if constexpr (WEIGHTED) re = kp.z * re, im = kp.z * im;
                            sample(h, al, sre, sim);
                            const float pr = re * sre, pi = im * sim; // product, then sum: two roundings each
                            acc_re[h] = acc_re[h] + pr;
                            acc_im[h] = acc_im[h] + pi;
                        }
                    };
                    // three registers in rotation: step al uses one while al+2 is loaded into the one
                    // step al-1 has just finished with
                    decltype(terms_of(0)) qa = terms_of(0), qb = terms_of(1), qc;
                    uint32_t al = 0;
                    for (; al + 2 < na; al += 3) {
                        qc = terms_of(al + 2);
                        products(al, qa);
                        qa = terms_of(al + 3);
                        products(al + 1, qb);
                        qb = terms_of(al + 4);
                        products(al + 2, qc);
                    }
                    if (al < na) products(al, qa);
                    if (al + 1 < na) products(al + 1, qb);
                });
            } else {
                // channel outermost and unrolled (h is a compile-time index: the accumulators stay in
                // registers, nothing goes to scratch), antennas in order inside -- the same sums
#pragma unroll
                for (int h = 0; h < CH; h++) {
                    float are = acc_re[h], aim = acc_im[h];
                    for (uint32_t al = 0; al < na; al++) {
                        const floatx2 kp = *reinterpret_cast<const floatx2 *>(tp + 2u * (uint64_t)(a0 + al) * a.B);
                        float re, im, sre, sim;
                        coeff_slow(kp.x, kp.y, fChan[h], D, re, im);
                        if constexpr (WEIGHTED) {
                            const float g = gp[(uint64_t)(a0 + al) * a.B];
                            re = g * re, im = g * im;
                        }
                        sample(h, al, sre, sim);
                        const float pr = re * sre, pi = im * sim;
                        are = are + pr;
                        aim = aim + pi;
                    }
                    acc_re[h] = are;
                    acc_im[h] = aim;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int h = 0; h < CH; h++) {
                if (c + h < cend) {
                    floatx2 *dst = reinterpret_cast<floatx2 *>(a.beams) +
                                   (((uint64_t)(c + h) * a.nt16_total + tex_g) * a.B + b) * 16u + t_in;
                    if constexpr (WEIGHTED) {
                        const float sb = w.gs[b];
                        *dst = floatx2{sb * acc_re[h], sb * acc_im[h]};
                    } else {
                        *dst = floatx2{acc_re[h], acc_im[h]};
                    }
                }
            }
        }
    }
}

