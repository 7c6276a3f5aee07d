// sg.hip — scatter-gather checksum batches (include/tulips_csum.h,
// tulips_csum_batch_sg & co.): a segment is the concatenation of fragments
// lying anywhere in memory (a header ring plus registered payload memory, NIC
// header-data split, a reassembly queue), and its result is the reference's
// utils::checksum (src/stack/Utils.cpp:14-42) and INET/TCP wrappers over the
// concatenated bytes.
//
// Combine rule (csum_common.h closed form). Fragment j at absolute address
// a_j, at logical offset x_j of its segment, with p_j = fold32 of its
// little-endian word sum taken at absolute addresses:
//   its big-endian contribution is p_j byte-swapped iff (a_j ^ x_j) is even.
// The kernel keeps the little-endian orientation instead (what finish()
// takes): q_j = p_j swapped iff (a_j ^ X_j) is odd, with X_j the fragment's
// byte offset in the WAVE's fragment run (x_j = X_j - X_first(segment)), and
// hands finish() the segment's sum of q_j with "start_odd" = X_first odd:
// all q_j of a segment that starts at an odd X are swapped together, which
// commutes with the sum (mod 65535, zero kept apart from 0xffff).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tulips_csum.h"
#include "csum_common.h"
#include "csum_device.h"
#include "csum_launch.h"

namespace tulips_amd {
namespace {

struct SgArgs
{
  const uint8_t* base;
  const uint64_t* foffs;
  const uint16_t* flens;
  uint32_t nfrags;
  const uint32_t* first; // n + 1 entries
  const uint16_t* seeds;
  const uint32_t* src;
  const uint32_t* dst;
  uint16_t* out;         // nullable when only counting
  uint32_t* bad;         // nullable: one uint32, zeroed before the launch
  uint32_t n;
  uint32_t mode;
};

// Little-endian partial (chunk_value sums, boundary bytes taken out) of one
// fragment per lane: lane j's fragment is [sa, sa + len), len == 0 for a lane
// without one. The packed chunk space of csum_packed_kernel
// (csum_kernels.hip) with a fragment per lane: the fragments' 16-byte chunk
// lists laid end to end, walked in double-buffered batches of U 64-chunk
// windows, each fragment's sum the difference of the running wave scan at
// its last chunk and at the previous fragment's. Every lane of every load
// carries a chunk of some fragment whatever the length mix (a 20 B header
// and a 1480 B payload cost 2-3 and 93-94 lane-loads). All loads
// unconditional; chunks past the end re-read the last one.
template<int U, bool NT>
__device__ __forceinline__ uint32_t
frag_partials(uintptr_t sa, uint32_t len, uint32_t lane)
{
  const uintptr_t zero_chunk = reinterpret_cast<uintptr_t>(k_zero_chunk);
  const uintptr_t a0 = sa & ~uintptr_t(15);
  const uint32_t nch = len ? uint32_t((sa + len - a0 + 15) >> 4) : 0u;
  const int head = int(sa - a0);
  const int tail = nch ? int(sa + len - a0) - 16 * int(nch - 1) : 16;
  // boundary chunks, only where bytes must be taken out (else a zero chunk)
  const gchunk_ptr pf = reinterpret_cast<gchunk_ptr>(
    (nch && head != 0) ? a0 : zero_chunk);
  const gchunk_ptr pl = reinterpret_cast<gchunk_ptr>(
    (nch && tail != 16) ? a0 + 16 * uintptr_t(nch - 1) : zero_chunk);
  const u32x4 cfirst = load_chunk<NT>(pf);
  const u32x4 clast = load_chunk<NT>(pl);
  const uint32_t incl = wave_incl_scan(nch);
  const uint32_t P = incl - nch;                  // first packed chunk
  const uint32_t T = __builtin_amdgcn_readlane(incl, 63);
  const uint32_t Lst = incl - 1;                  // last packed chunk
  const uint64_t D = uint64_t(a0) - 16ull * P;    // address = D + 16*c
  const uint64_t nonempty = __ballot(nch != 0);
  uint64_t pend_start = nonempty, pend_end = nonempty;
  uint64_t dcur = uint64_t(zero_chunk);           // D of the open fragment
  uint32_t run = 0;                               // R carried across windows
  uint32_t eprev = 0;                             // R at the previous end
  uint32_t sum = 0;                               // fragment sum (its lane)
  auto issue = [&](uint32_t w0, u32x4 (&v)[U]) {
    uint64_t addr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t b = w0 + 64u * u;
      // the fragment holding chunk b owns the window; fragments starting in
      // [b, b + 64) take over their lanes
      uint64_t dl = dcur;
      while (pend_start) {
        const uint32_t k = uint32_t(__builtin_ctzll(pend_start));
        const uint32_t pk = __builtin_amdgcn_readlane(P, k);
        if (pk >= b + 64u) {
          break;
        }
        pend_start &= pend_start - 1;
        const uint64_t dk = readlane64(D, k);
        dl = lane + b >= pk ? dk : dl;
        dcur = dk;
      }
      const uint32_t c = min(b + lane, T - 1u);   // past T: re-read, dropped
      addr[u] = dl + 16ull * c;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = load_chunk<NT>(reinterpret_cast<gchunk_ptr>(addr[u]));
    }
  };
  auto consume = [&](uint32_t w0, const u32x4 (&v)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t b = w0 + 64u * u;
      const uint32_t val = b + lane < T ? chunk_value(v[u]) : 0u;
      const uint32_t r = wave_incl_scan(val) + run;
      // fragments whose last chunk is in [b, b + 64): sum = R(end) - R(prev)
      while (pend_end) {
        const uint32_t k = uint32_t(__builtin_ctzll(pend_end));
        const uint32_t lk = __builtin_amdgcn_readlane(Lst, k);
        if (lk >= b + 64u) {
          break;
        }
        pend_end &= pend_end - 1;
        const uint32_t e = __builtin_amdgcn_readlane(r, lk - b);
        sum = lane == k ? e - eprev : sum;
        eprev = e;
      }
      run = __builtin_amdgcn_readlane(r, 63);
    }
  };
  if (T != 0) {
    u32x4 cur[U];
    issue(0, cur);
    uint32_t w0 = 0;
    for (; w0 + 64u * U < T; w0 += 64u * U) {
      u32x4 nxt[U];
      issue(w0 + 64u * U, nxt);
      consume(w0, cur);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        cur[u] = nxt[u];
      }
    }
    consume(w0, cur);
  }
  const uint32_t outside =
    masked_value(cfirst, 0, head) + masked_value(clast, tail, 16);
  return sum - outside;
}

// ---------------------------------------------------------------------------
// Segment-major scatter-gather kernel. A wave owns S consecutive segments;
// their fragments are consecutive in the plan (seg_first is a CSR row
// pointer), so no segment spans two waves and nothing meets in memory. The
// wave walks its fragment run in batches of at most 64, one fragment's
// metadata per lane (coalesced loads), and sums each batch on the packed
// chunk space above. Per batch, two wave scans carried across batches:
//   X = bytes before each fragment (its logical parity, the TCP length),
//   A = sum of the normalised 16-bit fragment partials q.
// Segment k's sum and length are second differences of those prefixes at
// fragment indices seg_first[k] and seg_first[k+1]; a scalar cursor over the
// wave's S + 1 boundaries picks them out with v_readlane as the batches pass
// (a segment spanning batches just has its two boundaries in different
// batches) and parks them in lane k. u32 arithmetic wraps; the differences
// are exact because a segment has < 2^16 non-empty fragments of < 2^16 each.
//
// Out of contract (seg_first not monotone or past nfrags, a segment longer
// than 65535): unspecified results for those segments. Metadata indices are
// clamped to [0, nfrags) / [0, n], the batch loop runs over a clamped,
// non-negative count, and data is read only inside the 16-byte hull of
// fragments in [seg_first[g0], seg_first[g0 + S)).
// ---------------------------------------------------------------------------
template<int S, int U, bool NT>
__global__ __launch_bounds__(1024) void
csum_sg_kernel(SgArgs a)
{
  static_assert(S >= 1 && S <= 63, "S + 1 boundaries in one wave");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(
    (xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x) >> 6);
  const uint64_t gstride = uint64_t((gridDim.x * blockDim.x) >> 6) * S;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.base);
  const gu32_ptr first = reinterpret_cast<gu32_ptr>(reinterpret_cast<uintptr_t>(a.first));
  const gu64_ptr foffs = reinterpret_cast<gu64_ptr>(reinterpret_cast<uintptr_t>(a.foffs));
  const gu16_ptr flens = reinterpret_cast<gu16_ptr>(reinterpret_cast<uintptr_t>(a.flens));
  uint32_t nbad = 0;
  for (uint64_t g = uint64_t(wave) * S; g < a.n; g += gstride) {
    const uint32_t g0 = uint32_t(g);
    const uint32_t ns = min(uint32_t(S), a.n - g0);     // segments of this wave
    // lane k <= ns: boundary k = seg_first[g0 + k]; lane k < ns: segment g0 + k
    const uint32_t F = min(first[g0 + min(lane, ns)], a.nfrags);
    const bool mine = lane < ns;
    const uint32_t seg = mine ? g0 + lane : g0;
    const SideIn side = load_side(seg, a.seeds, a.src, a.dst, a.mode);
    const uint32_t f_begin = __builtin_amdgcn_readlane(F, 0);
    const uint32_t f_end = __builtin_amdgcn_readlane(F, ns);
    uint32_t fb = f_begin;
    uint32_t rem = f_end > f_begin ? f_end - f_begin : 0u;
    uint32_t kb = 0;                       // next boundary to place
    uint32_t carry_a = 0, carry_x = 0;     // prefixes at fragment fb
    uint32_t start_a = 0, end_a = 0, start_x = 0, end_x = 0;
    while (rem != 0) {
      const uint32_t nb = min(rem, 64u);
      const bool act = lane < nb;
      const uint32_t fi = act ? fb + lane : fb;      // fb < f_end <= nfrags
      const uint32_t len = act ? uint32_t(flens[fi]) : 0u;
      const uintptr_t sa = base + foffs[fi];
      const uint32_t p = fold32(frag_partials<U, NT>(sa, len, lane));
      const uint32_t xi = wave_incl_scan(len) + carry_x;
      const uint32_t x = xi - len;
      const uint32_t q = ((uint32_t(sa) ^ x) & 1u) ? bswap16(p) : p;
      const uint32_t ai = wave_incl_scan(q) + carry_a;
      // boundaries at fragment index in [fb, fb + nb]: exclusive prefixes
      while (kb <= ns) {
        const uint32_t d = __builtin_amdgcn_readlane(F, kb) - fb;
        if (d > nb) {
          break;
        }
        const uint32_t dl = d ? d - 1u : 0u;
        const uint32_t ra = __builtin_amdgcn_readlane(ai, dl);
        const uint32_t rx = __builtin_amdgcn_readlane(xi, dl);
        const uint32_t va = d ? ra : carry_a, vx = d ? rx : carry_x;
        start_a = lane == kb ? va : start_a;
        start_x = lane == kb ? vx : start_x;
        end_a = lane + 1u == kb ? va : end_a;
        end_x = lane + 1u == kb ? vx : end_x;
        ++kb;
      }
      carry_a = __builtin_amdgcn_readlane(ai, 63);
      carry_x = __builtin_amdgcn_readlane(xi, 63);
      fb += nb;
      rem -= nb;
    }
    const uint32_t r = finish(end_a - start_a, (start_x & 1u) != 0, a.mode, side.seed,
                              side.src, side.dst, end_x - start_x);
    if (mine && a.out) {
      a.out[seg] = uint16_t(r);
    }
    const bool isbad = mine && (r ^ ((a.mode & FLAG_COMPLEMENT) ? 0u : 0xffffu)) != 0;
    nbad += uint32_t(__popcll(__ballot(isbad)));
  }
  // one wave-aggregated atomic
  if (a.bad && lane == 0 && nbad != 0) {
    atomicAdd(a.bad, nbad);
  }
}

template<int S, int U, bool NT>
hipError_t
launch_sg_one(const SgArgs& a, int block, hipStream_t stream)
{
  const uint64_t per_block = uint64_t(block / 64) * S;
  const uint64_t blocks = (uint64_t(a.n) + per_block - 1) / per_block;
  (void)hipGetLastError();
  hipLaunchKernelGGL((csum_sg_kernel<S, U, NT>), dim3(uint32_t(blocks)), dim3(block), 0,
                     stream, a);
  return hipGetLastError();
}

// The shipped instances: S segments per wave x U 64-chunk windows per batch.
constexpr int SG_DEFAULT_S = 8, SG_DEFAULT_U = 4;

hipError_t
launch_sg(const SgArgs& a, int s, int u, bool nt, int block, hipStream_t stream)
{
#define TCS_SGCASE(S_, U_)                                                     \
  if (s == S_ && u == U_) {                                                    \
    return nt ? launch_sg_one<S_, U_, true>(a, block, stream)                  \
              : launch_sg_one<S_, U_, false>(a, block, stream);                \
  }
  TCS_SGCASE(8, 2)
  TCS_SGCASE(8, 4)
  TCS_SGCASE(16, 2)
  TCS_SGCASE(16, 4)
#undef TCS_SGCASE
  return hipErrorInvalidValue;
}

inline bool
sg_mode_ok(uint32_t mode, const uint32_t* src, const uint32_t* dst)
{
  if ((mode & ~(TULIPS_CSUM_MODE_MASK | TULIPS_CSUM_COMPLEMENT)) != 0) {
    return false;
  }
  const uint32_t m = mode & TULIPS_CSUM_MODE_MASK;
  return m <= TULIPS_CSUM_TCP && (m != TULIPS_CSUM_TCP || (src && dst));
}

// n > 0. bad (nullable) is zeroed on the stream before the launch.
int
sg_device(const uint8_t* base, const uint64_t* frag_offsets, const uint16_t* frag_lengths,
          uint32_t nfrags, const uint32_t* seg_first, const uint16_t* seeds,
          const uint32_t* src, const uint32_t* dst, uint16_t* out, uint32_t* bad, uint32_t n,
          uint32_t mode, const tulips_csum_tuning* t, void* stream)
{
  if (!seg_first || (!out && !bad) || !sg_mode_ok(mode, src, dst) ||
      (nfrags && (!base || !frag_offsets || !frag_lengths))) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  const int s = (t && t->group) ? t->group : SG_DEFAULT_S;
  const int u = (t && t->unroll) ? t->unroll : SG_DEFAULT_U;
  const bool nt = ((t && t->nontemporal >= 0) ? t->nontemporal : 1) & 1;
  const int block = (t && t->block) ? t->block : 256;
  if (block != 256 && block != 512 && block != 1024) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (bad) {
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) {
      return status_of_hip(e);
    }
  }
  const SgArgs a{base, frag_offsets, frag_lengths, nfrags, seg_first, seeds, src, dst,
                 out, bad, n, mode};
  return status_of_hip(launch_sg(a, s, u, nt, block, st));
}

// Host: little-endian dword sum of data[0, len) relative to `data`, folded.
inline uint32_t
sg_host_partial(const uint8_t* data, uint32_t len)
{
  uint64_t acc = 0;
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t w;
    memcpy(&w, data + i, 8);
    acc += (w & 0xffffffffu) + (w >> 32);
  }
  if (i < len) {
    uint64_t w = 0;
    memcpy(&w, data + i, len - i);
    acc += (w & 0xffffffffu) + (w >> 32);
  }
  return fold32(fold64(acc));
}

} // namespace
} // namespace tulips_amd

using namespace tulips_amd;

extern "C" {

int
tulips_csum_batch_sg(const uint8_t* base, const uint64_t* frag_offsets,
                     const uint16_t* frag_lengths, uint32_t nfrags,
                     const uint32_t* seg_first, const uint16_t* seeds, const uint32_t* src,
                     const uint32_t* dst, uint16_t* out, uint32_t n, uint32_t mode,
                     void* stream)
{
  if (n == 0) {
    return TULIPS_STATUS_OK;
  }
  if (!out) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  return sg_device(base, frag_offsets, frag_lengths, nfrags, seg_first, seeds, src, dst, out,
                   nullptr, n, mode, nullptr, stream);
}

int
tulips_csum_batch_sg_tuned(const uint8_t* base, const uint64_t* frag_offsets,
                           const uint16_t* frag_lengths, uint32_t nfrags,
                           const uint32_t* seg_first, const uint16_t* seeds,
                           const uint32_t* src, const uint32_t* dst, uint16_t* out,
                           uint32_t n, uint32_t mode, const tulips_csum_tuning* tuning,
                           void* stream)
{
  if (n == 0) {
    return TULIPS_STATUS_OK;
  }
  if (!out) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  return sg_device(base, frag_offsets, frag_lengths, nfrags, seg_first, seeds, src, dst, out,
                   nullptr, n, mode, tuning, stream);
}

int
tulips_csum_verify_sg(const uint8_t* base, const uint64_t* frag_offsets,
                      const uint16_t* frag_lengths, uint32_t nfrags,
                      const uint32_t* seg_first, const uint32_t* src, const uint32_t* dst,
                      uint16_t* out, uint32_t* bad_count, uint32_t n, uint32_t mode,
                      void* stream)
{
  const uint32_t m = mode & TULIPS_CSUM_MODE_MASK;
  if (!bad_count || (m != TULIPS_CSUM_INET && m != TULIPS_CSUM_TCP)) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  if (n == 0) {
    return status_of_hip(
      hipMemsetAsync(bad_count, 0, sizeof(uint32_t), static_cast<hipStream_t>(stream)));
  }
  return sg_device(base, frag_offsets, frag_lengths, nfrags, seg_first, nullptr, src, dst,
                   out, bad_count, n, mode, nullptr, stream);
}

int
tulips_csum_batch_sg_cpu(const uint8_t* base, const uint64_t* frag_offsets,
                         const uint16_t* frag_lengths, uint32_t nfrags,
                         const uint32_t* seg_first, const uint16_t* seeds,
                         const uint32_t* src, const uint32_t* dst, uint16_t* out,
                         uint32_t* bad_count, uint32_t n, uint32_t mode)
{
  // (a rejected call writes nothing: bad_count is stored only on success)
  if (n == 0) {
    if (bad_count) {
      *bad_count = 0;
    }
    return TULIPS_STATUS_OK;
  }
  if (!seg_first || (!out && !bad_count) || !sg_mode_ok(mode, src, dst) ||
      (nfrags && (!base || !frag_offsets || !frag_lengths))) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  // the plan: non-decreasing, inside [0, nfrags]
  for (uint32_t i = 0; i < n; ++i) {
    if (seg_first[i] > seg_first[i + 1]) {
      return TULIPS_STATUS_INVALID_ARGUMENT;
    }
  }
  if (seg_first[n] > nfrags) {
    return TULIPS_STATUS_INVALID_ARGUMENT;
  }
  const uint32_t ok = (mode & TULIPS_CSUM_COMPLEMENT) ? 0u : 0xffffu;
  uint32_t nbad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t acc = 0;   // big-endian oriented 16-bit partials, plain integers
    uint32_t x = 0;     // logical offset
    for (uint32_t j = seg_first[i]; j < seg_first[i + 1]; ++j) {
      const uint32_t len = frag_lengths[j];
      const uint32_t p = sg_host_partial(base + frag_offsets[j], len);
      acc = fold32(acc + ((x & 1u) ? p : bswap16(p)));
      x += len;
    }
    // (acc is already big-endian: finish() must not swap again)
    const uint32_t r = finish(acc, true, mode, seeds ? seeds[i] : 0u, src ? src[i] : 0u,
                              dst ? dst[i] : 0u, x);
    if (out) {
      out[i] = uint16_t(r);
    }
    nbad += r != ok ? 1u : 0u;
  }
  if (bad_count) {
    *bad_count = nbad;
  }
  return TULIPS_STATUS_OK;
}

} // extern "C"
