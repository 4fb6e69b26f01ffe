// waterfall: the short-time spectra of every channel's staged hop (msk144_set_wideband_waterfall, include/msk144hip.h).
//
// Per channel the work is one complex GEMM, rows[b][j] = |sum_i x[96b + i] . W[j][i]|^2 with the 96 x 96 windowed DFT matrix
// W[j][i] = w[i] e^{-j2pi i k/96}, k = (j - 48) mod 96 (formed in double on the host, stored f32) and the channel's 96 x nb block
// matrix, nb = 27 blocks of a hop or 54 of a first push.  It runs in the channeliser's idiom: v_mfma_f32_32x32x2_f32 with the two
// k-slots of the instruction carrying the real and the imaginary part, int8 being exact in f32:
//     A[b][0] = Re x, A[b][1] = Im x;   Re: B[0][j] = Re W, B[1][j] = -Im W;   Im: B[0][j] = Im W, B[1][j] = Re W
// The samples are the A operand and the matrix the B operand, so that an accumulator has the block b in its registers and the
// slot j on its lanes: a register of |X|^2 is stored as two runs of 32 consecutive floats of two rows.
//
// One workgroup = one channel = 3 waves, wave t on slots 32t .. 32t + 31, each over all blocks: 27 pad to one tile of 32 columns, 54
// to two, so 96 steps of 2 or 4 MFMAs per wave, 576 or 1152 per channel.  The hop is staged once in LDS as f32, [re/im][i][b] with
// an odd row stride: consecutive threads write consecutive i (odd stride: distinct banks), a half-wave reads 32 consecutive b, and
// the imaginary plane lies 32 banks from the real one.  The matrix streams from L2 in the order the loop walks, 256 contiguous
// bytes per step and wave (73 KB for all three waves, shared by every channel).  Workgroups are indexed by channel, so the padded
// slots of a bank rate do not enter.  A second kernel adds a channel's rows in ascending b in double.  No atomics, no scratch, and
// no order between workgroups: the same hops give the same bytes.
#include "msk144_kernels.h"

namespace msk144
{

namespace
{

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBins = msk144wb::kWaterfallBins;               // 96
constexpr int kRows = msk144wb::kWaterfallRows;               // 54
constexpr int kWaves = kBins / 32;                            // 3
constexpr int kHopBlocks = kHopSamples / kBins;               // 27
constexpr int kRowBytes = 2 * kHopSamples;                    // a channel's row of first_halves or hops
static_assert(kBins % 32 == 0 && kHopSamples % kBins == 0 && 2 * kHopBlocks == kRows && kHopBlocks <= 32, "a hop is 27 whole blocks: one tile of 32 columns");

// NBT: tiles of 32 blocks, 1 for a hop and 2 for a first push (its first 27 blocks in first_halves, the others in hops)
template<int NBT>
__global__ __launch_bounds__(kWaves * 64) void waterfall_kernel(const int8_t* __restrict__ first_halves, const int8_t* __restrict__ hops, const float2* __restrict__ dft,
                                                                float* __restrict__ rows)
{
    constexpr int kStride = 32 * NBT + 1;
    constexpr int nb = kHopBlocks * NBT;
    static_assert((kBins * kStride) % 64 == 32, "the imaginary plane lies 32 banks from the real one");
    __shared__ float xs[2][kBins][kStride];

    const int ch = blockIdx.x;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int col = lane & 31;
    const int hsel = lane >> 5;  // k-slot of the MFMA: 0 = real part, 1 = imaginary part

    // sample s = 96 b + i of the push to xs[.][i][b]; the columns past nb are 0
    const char2* __restrict__ head = reinterpret_cast<const char2*>((NBT == 2 ? first_halves : hops) + static_cast<size_t>(ch) * kRowBytes);
    const char2* __restrict__ tail = reinterpret_cast<const char2*>(hops + static_cast<size_t>(ch) * kRowBytes);
    for(int s = threadIdx.x; s < 32 * NBT * kBins; s += kWaves * 64)
    {
        const int b = s / kBins;
        const int i = s - b * kBins;
        char2 v = make_char2(0, 0);
        if(b < kHopBlocks) v = head[s];
        else if(b < nb) v = tail[s - kHopSamples];
        xs[0][i][b] = static_cast<float>(v.x);
        xs[1][i][b] = static_cast<float>(v.y);
    }
    __syncthreads();

    f32x16 acc_re[NBT] = {}, acc_im[NBT] = {};
    const float2* __restrict__ w = dft + static_cast<size_t>(wave) * kBins * 32 + col;
    const float* xr = &xs[hsel][0][col];
#pragma unroll 8
    for(int i = 0; i < kBins; i++)
    {
        const float2 wv = w[i * 32];
        const float b_re = hsel ? -wv.y : wv.x;
        const float b_im = hsel ? wv.x : wv.y;
#pragma unroll
        for(int t = 0; t < NBT; t++)
        {
            const float a = xr[i * kStride + 32 * t];
            acc_re[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_re, acc_re[t], 0, 0, 0);
            acc_im[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_im, acc_im[t], 0, 0, 0);
        }
    }

    // D[row][col]: col = lane & 31 = slot within the wave, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = block within the tile
    float* __restrict__ out = rows + static_cast<size_t>(ch) * kRows * kBins + wave * 32 + col;
#pragma unroll
    for(int t = 0; t < NBT; t++)
    {
#pragma unroll
        for(int r = 0; r < 16; r++)
        {
            const int b = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hsel;
            if(b < nb) out[b * kBins] = acc_re[t][r] * acc_re[t][r] + acc_im[t][r] * acc_im[t][r];
        }
    }
}

// sums[ch][j] = the f32 rows of the channel added one after another in double, b ascending
__global__ __launch_bounds__(kBins) void waterfall_sums_kernel(const float* __restrict__ rows, int nb, double* __restrict__ sums)
{
    const int ch = blockIdx.x;
    const int j = threadIdx.x;
    const float* __restrict__ src = rows + static_cast<size_t>(ch) * kRows * kBins + j;
    double s = 0.0;
    for(int b = 0; b < nb; b++) s += static_cast<double>(src[b * kBins]);
    sums[static_cast<size_t>(ch) * kBins + j] = s;
}

}  // namespace

void launch_waterfall(const int8_t* first_halves, const int8_t* hops, int first, int channels, const float2* dft, float* rows, double* sums, hipStream_t stream)
{
    if(first) hipLaunchKernelGGL(waterfall_kernel<2>, dim3(channels), dim3(kWaves * 64), 0, stream, first_halves, hops, dft, rows);
    else hipLaunchKernelGGL(waterfall_kernel<1>, dim3(channels), dim3(kWaves * 64), 0, stream, first_halves, hops, dft, rows);
    hipLaunchKernelGGL(waterfall_sums_kernel, dim3(channels), dim3(kBins), 0, stream, rows, first ? kRows : kHopBlocks, sums);
}

}  // namespace msk144
