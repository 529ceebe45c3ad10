// dgraph_amd — fused per-edge dot products (SDDMM) over a CSR pattern for gfx950.
//
//   s[k, h] = scale * row_scale[r(k)] * sum_{d < D} a[r(k), h D + d] * b[col[k], h D + d]
//
// for every CSR slot k, r(k) the row that holds it, D = F / heads; a and b fp32 or bf16 (the
// same), each with its own row stride, fp32 accumulation, s contiguous fp32 [nnz, heads].
// Composed from two row gathers and a product this is two [nnz, F] tensors; here nothing per
// edge but the scores is written. It is the edge-weight gradient of the weighted SpMM
// (a = dL/dout, b = x) and the score of a link-prediction decoder (a = b = z).
//
// Mapping: SLOT-parallel, not row-parallel. Nothing is reduced along a row, so rows do not
// shape the work at all: the (slot, head) pairs u = k heads + h are cut into equal chunks
// (sddmm_chunk_slots slots), a wave takes chunks in grid-stride order, and inside a chunk a
// block of L lanes owns one pair at a time, G = 64 / L pairs per pass and KU passes in flight
// (the kU pattern of dot_attn_f32.hip: all of a batch's column ids are loaded, then all of its
// rows). A 5,000-entry row and 5,000 rows of one entry are the same number of batches.
//
// The row of a slot: ONE search of rowptr per chunk, then a walk. The search is 64-ary and
// wave-cooperative (each lane probes one row pointer, a ballot picks the sub-range: 4 steps
// for 10^7 rows where a bisection has 24 dependent loads), the walk is per lane
// (`while (k >= row_end) ++row`), skips empty rows, and loads nothing while the slots stay in
// one row. A cached int32 row-id array on the CSR was the alternative: it costs 4 B per slot
// of traffic against the 4 B col id and the 4 heads B score that are all this kernel moves per
// slot besides the rows, and 0.5 GB resident per CSR at the ogbn-products shape (its
// transposes and blocks included); the search costs four loads per 512 slots.
//
// a's segment of a (row, head) is resident in registers and reloaded only when the lane's
// (row, head) changes: never inside a long row, once per slot on degree-1 rows. The reload is
// issued with the batch's gathers, not after them.
//
// Paths (sddmm_vec_shape_ok says which one a shape takes):
// * vector: D % 4 == 0, D / 4 a power of two, D <= 1024. Four elements per lane and access
//   (16 B fp32, 8 B bf16): bases aligned to four elements, row strides divisible by 4
//   (checked in bindings_sddmm.cpp). Heads are aligned blocks of L = min(D / 4, 64) lanes;
//   a head wider than one wave's 256 columns (D = 512, 1024) loops over NB = 2, 4 column
//   blocks with its partial sum and its a-segment in registers (KU = 8 / NB).
// * generic: every other F >= 1 and heads dividing F, one element per lane and access, no
//   alignment assumed. D <= 64: L = the power of two >= D (lanes past D hold zeros), a
//   resident as above. D > 64: L = 64 and a run-time loop over ceil(D / 64) column blocks
//   with the partial sums in registers; a's elements are then loaded next to b's (an
//   L1 / L2 hit after the first slot of a row), since a run-time-wide segment has no
//   registers to stay in.
//
// Summation order of one score, fixed: a lane's own terms in column order as fma's from the
// first product, then the xor tree of head_sum over the L lanes. No atomics, no LDS; the same
// for int32 and int64 column ids, so the two are bitwise equal, as are two runs.
//
// A launch needs nnz >= 1 and nrows >= 1 (the launcher returns before that), rowptr[0] == 0
// and rowptr[nrows] == nnz; the walk is bounded by nrows whatever rowptr holds. Column ids
// are the caller's contract, as for spmm_csr.
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; no LDS, no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD =
// min(8, 512 / VGPRs); all 68 instantiations: 17 (VEC, L, NB) x fp32 / bf16 x int32 / int64,
// the index widths within 1 VGPR of each other):
//   vector, NB = 1 (L = 1 .. 64)   100 .. 116 VGPRs   scratch 0 B   occupancy 4
//     (8 a-vectors and 8 gathered b-vectors of four elements in flight)
//   vector, NB = 2 / 4              95 .. 102 VGPRs   scratch 0 B   occupancy 4 (bf16 NB = 4: 5)
//   generic, D <= 64 (L = 1 .. 64)  73 ..  94 VGPRs   scratch 0 B   occupancy 5 .. 6
//   generic, D > 64 (run-time loop)       68 VGPRs   scratch 0 B   occupancy 7
// The grid cap of 2048 workgroups is 8 waves per SIMD on 256 CUs: at least every kernel's
// occupancy, and the chunks past it are taken in grid-stride order.
#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int64_t kGridCap = 2048;  // workgroups of 4 waves: 8 per CU on 256 CUs
constexpr int kChunkMax = 512;      // slots per chunk (one rowptr search each)

struct SddmmArgs {
  const int64_t* rowptr;
  const void* col;
  int64_t nrows;
  int64_t nnz;
  const void* a;
  int64_t lda;
  const void* b;
  int64_t ldb;
  const float* row_scale;  // [nrows] or nullptr (== 1)
  float scale;
  float* s;                // [nnz, heads] contiguous
  int heads;
  int hshift;              // log2(heads), or -1 when heads is no power of two
  int D;
  int nblk;                // column blocks of L lanes per head (the run-time loop's count)
  int chunk;               // slots per chunk
};

// sum over the L lanes of one head (contiguous, aligned lane blocks); the same in all of them
template <int L>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int off = L / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// this lane's VEC terms of <a, b> on top of p (p == 0 and first: the plain product starts it,
// dot_attn_f32.hip's dot4)
template <int VEC>
__device__ __forceinline__ float dotv(const float (&a)[VEC], const float (&b)[VEC], float p,
                                      bool first) {
  p = first ? a[0] * b[0] : fmaf(a[0], b[0], p);
#pragma unroll
  for (int i = 1; i < VEC; ++i) p = fmaf(a[i], b[i], p);
  return p;
}

// The last row r with rowptr[r] <= k (the row that holds slot k, since k < rowptr[nrows]):
// a 64-ary search by the whole wave. Invariant: rowptr[lo] <= k and the answer is in
// [lo, lo + n). Every lane of the wave must be active.
__device__ __forceinline__ int64_t find_row(const int64_t* __restrict__ rowptr, int64_t nrows,
                                            int64_t k, int lane) {
  int64_t lo = 0, n = nrows;
  while (n > 1) {
    const int64_t step = (n + kWave - 1) >> 6;
    const int64_t hi = lo + n;
    const int64_t idx = lo + (lane + 1) * step;
    const bool le = idx < hi && rowptr[idx] <= k;  // a prefix of the lanes; never all 64
    lo += __popcll(__ballot(le)) * step;
    n = hi - lo < step ? hi - lo : step;
  }
  return lo;
}

// NB > 0: NB column blocks per head, a resident; NB == 0: p.nblk blocks at run time
template <typename T, typename IdxT, int VEC, int L, int NB>
__global__ __launch_bounds__(256) void sddmm_kernel(SddmmArgs p) {
  constexpr bool RESIDENT = NB > 0;
  constexpr int NBC = RESIDENT ? NB : 1;
  constexpr int G = kWave / L;                  // (slot, head) pairs per pass
  constexpr int KU = RESIDENT ? 8 / NB : 4;     // passes in flight
  constexpr int UB = G * KU;                    // pairs per batch
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / L, l = lane % L;
  const T* __restrict__ A = static_cast<const T*>(p.a);
  const T* __restrict__ B = static_cast<const T*>(p.b);
  const IdxT* __restrict__ col = static_cast<const IdxT*>(p.col);
  const int heads = p.heads, D = p.D;
  const int64_t w0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t wstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t nchunks = (p.nnz + p.chunk - 1) / p.chunk;
  for (int64_t c = w0; c < nchunks; c += wstep) {
    const int64_t k0 = c * p.chunk;
    const int64_t kend = k0 + p.chunk < p.nnz ? k0 + p.chunk : p.nnz;
    const int nun = static_cast<int>(kend - k0) * heads;  // pairs of this chunk
    const int64_t rbase = find_row(p.rowptr, p.nrows, k0, lane);
    int ro = 0;                                  // this lane's row, as rbase + ro
    int64_t rend = p.rowptr[rbase + 1];
    int cur_r = -1, cur_h = -1;                  // the (row, head) whose a-segment is resident
    float av[NBC][VEC];
#pragma unroll
    for (int nb = 0; nb < NBC; ++nb)
#pragma unroll
      for (int i = 0; i < VEC; ++i) av[nb][i] = 0.f;
    for (int ub = 0; ub < nun; ub += UB) {
      // the batch's pairs: slot, head, row (the walk) and column id
      int ru[KU], hu[KU];
      IdxT cu[KU];
      bool ok[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int lu = ub + u * G + g;
        ok[u] = lu < nun;
        const int lk = p.hshift >= 0 ? lu >> p.hshift : lu / heads;
        hu[u] = lu - lk * heads;
        const int64_t k = k0 + lk;
        if (ok[u]) {
          while (k >= rend && rbase + ro + 1 < p.nrows) {
            ++ro;
            rend = p.rowptr[rbase + ro + 1];
          }
        }
        ru[u] = ro;
        cu[u] = ok[u] ? col[k] : static_cast<IdxT>(0);
      }
      float rs[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u)
        rs[u] = (ok[u] && p.row_scale) ? p.row_scale[rbase + ru[u]] : 1.f;
      float sum[KU];
      if constexpr (RESIDENT) {
        float au[KU][NBC][VEC], bu[KU][NBC][VEC];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          const bool fresh = ok[u] && (ru[u] != cur_r || hu[u] != cur_h);
          const T* ap = A + (rbase + ru[u]) * p.lda + hu[u] * D;
          const T* bp = B + static_cast<int64_t>(cu[u]) * p.ldb + hu[u] * D;
#pragma unroll
          for (int nb = 0; nb < NBC; ++nb) {
            const int d = (nb * L + l) * VEC;
            const bool in = VEC > 1 || d < D;  // the vector path has no partial block
            if (fresh) {
              if (in) {
                load_vec_f32<T, VEC>(ap + d, av[nb]);
              } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) av[nb][i] = 0.f;
              }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              au[u][nb][i] = av[nb][i];
              bu[u][nb][i] = 0.f;
            }
            if (ok[u] && in) load_vec_f32<T, VEC>(bp + d, bu[u][nb]);
          }
          if (fresh) {
            cur_r = ru[u];
            cur_h = hu[u];
          }
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          float acc = 0.f;
#pragma unroll
          for (int nb = 0; nb < NBC; ++nb) acc = dotv<VEC>(au[u][nb], bu[u][nb], acc, nb == 0);
          sum[u] = acc;
        }
      } else {
#pragma unroll
        for (int u = 0; u < KU; ++u) sum[u] = 0.f;
        for (int cb = 0; cb < p.nblk; ++cb) {
          const int d = (cb * L + l) * VEC;
          const bool in = d < D;
          float au[KU][VEC], bu[KU][VEC];
#pragma unroll
          for (int u = 0; u < KU; ++u) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) au[u][i] = bu[u][i] = 0.f;
            if (ok[u] && in) {
              load_vec_f32<T, VEC>(A + (rbase + ru[u]) * p.lda + hu[u] * D + d, au[u]);
              load_vec_f32<T, VEC>(B + static_cast<int64_t>(cu[u]) * p.ldb + hu[u] * D + d,
                                   bu[u]);
            }
          }
#pragma unroll
          for (int u = 0; u < KU; ++u) sum[u] = dotv<VEC>(au[u], bu[u], sum[u], cb == 0);
        }
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const float tot = head_sum<L>(sum[u]);
        if (ok[u] && l == 0)
          p.s[k0 * heads + (ub + u * G + g)] = p.scale * rs[u] * tot;
      }
    }
  }
}

// how a shape runs: VEC elements per lane, L lanes per head, NB resident blocks (0: the
// run-time loop of nblk blocks), and the pairs of one batch
struct Plan {
  int vec, L, NB, nblk, batch;
};

bool vec_ok(int F, int heads) {
  if (F <= 0 || heads <= 0 || F % heads != 0) return false;
  const int D = F / heads;
  if (D % 4 != 0 || D > 1024) return false;
  const int q = D / 4;
  return (q & (q - 1)) == 0;
}

Plan plan_of(int F, int heads) {
  const int D = F / heads;
  Plan pl{};
  if (vec_ok(F, heads)) {
    const int q = D / 4;
    pl.vec = 4;
    pl.L = q < kWave ? q : kWave;
    pl.NB = q / pl.L;
    pl.nblk = pl.NB;
  } else {
    pl.vec = 1;
    int L = 1;
    while (L < D && L < kWave) L <<= 1;
    pl.L = L;
    pl.NB = D <= kWave ? 1 : 0;
    pl.nblk = (D + L - 1) / L;
  }
  const int ku = pl.NB > 0 ? 8 / pl.NB : 4;
  pl.batch = kWave / pl.L * ku;
  return pl;
}

int chunk_of(const Plan& pl, int heads) {
  const int one = (pl.batch + heads - 1) / heads;  // slots of one batch
  int many = 16 * pl.batch / heads;
  if (many > kChunkMax) many = kChunkMax;
  return one > many ? one : many;
}

template <typename T, typename IdxT>
hipError_t launch_typed(const SddmmArgs& a, const Plan& pl, hipStream_t st) {
  const int64_t nchunks = (a.nnz + a.chunk - 1) / a.chunk;
  const dim3 grid(static_cast<unsigned>(cap_blocks((nchunks + 3) / 4, kGridCap))), block(256);
#define DG_SDDMM(V_, L_, NB_)                                                            \
  if (pl.vec == V_ && pl.L == L_ && pl.NB == NB_) {                                      \
    hipLaunchKernelGGL((sddmm_kernel<T, IdxT, V_, L_, NB_>), grid, block, 0, st, a);     \
    return hipGetLastError();                                                            \
  }
  DG_SDDMM(4, 1, 1) DG_SDDMM(4, 2, 1) DG_SDDMM(4, 4, 1) DG_SDDMM(4, 8, 1)
  DG_SDDMM(4, 16, 1) DG_SDDMM(4, 32, 1) DG_SDDMM(4, 64, 1) DG_SDDMM(4, 64, 2)
  DG_SDDMM(4, 64, 4)
  DG_SDDMM(1, 1, 1) DG_SDDMM(1, 2, 1) DG_SDDMM(1, 4, 1) DG_SDDMM(1, 8, 1)
  DG_SDDMM(1, 16, 1) DG_SDDMM(1, 32, 1) DG_SDDMM(1, 64, 1) DG_SDDMM(1, 64, 0)
#undef DG_SDDMM
  return hipErrorInvalidValue;
}

}  // namespace

bool sddmm_vec_shape_ok(int F, int heads) { return vec_ok(F, heads); }

int64_t sddmm_grid_cap() { return kGridCap; }

int64_t sddmm_chunk_slots(int F, int heads) {
  if (F <= 0 || heads <= 0 || F % heads != 0) return 0;
  return chunk_of(plan_of(F, heads), heads);
}

hipError_t sddmm_csr(DType dt, IType it, const int64_t* rowptr, const void* col, int64_t nrows,
                     int64_t nnz, const void* a, int64_t lda, const void* b, int64_t ldb,
                     int F, int heads, float scale, const float* row_scale, float* s,
                     hipStream_t st) {
  if (nnz <= 0 || nrows <= 0 || F <= 0) return hipSuccess;
  if (heads <= 0 || F % heads != 0 || nrows > 0x7fffffff) return hipErrorInvalidValue;
  const Plan pl = plan_of(F, heads);
  SddmmArgs p{};
  p.rowptr = rowptr;
  p.col = col;
  p.nrows = nrows;
  p.nnz = nnz;
  p.a = a;
  p.lda = lda;
  p.b = b;
  p.ldb = ldb;
  p.row_scale = row_scale;
  p.scale = scale;
  p.s = s;
  p.heads = heads;
  p.hshift = -1;
  for (int sft = 0; sft < 31; ++sft)
    if ((1 << sft) == heads) p.hshift = sft;
  p.D = F / heads;
  p.nblk = pl.nblk;
  p.chunk = chunk_of(pl, heads);
  if (dt == DType::F32)
    return it == IType::I32 ? launch_typed<float, int32_t>(p, pl, st)
                            : launch_typed<float, int64_t>(p, pl, st);
  return it == IType::I32 ? launch_typed<uint16_t, int32_t>(p, pl, st)
                          : launch_typed<uint16_t, int64_t>(p, pl, st);
}

}  // namespace dgraph
