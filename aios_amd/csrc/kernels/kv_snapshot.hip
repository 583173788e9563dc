// KV snapshot (ops.h KvSnapArgs): gather one slot's cached positions [0, n) of every layer through the slot's row
// of the device block table into one contiguous buffer [layer][K, V][kv_head][token][head_dim] (pack), or scatter
// such a buffer back into the slot's mapped blocks (unpack).  Bytes move verbatim: no conversion for bf16 or fp8.
//
//  - One launch for every layer, either direction: workgroup (block j of the row x kv head, K or V, layer) owns
//    the rows of block j that are below n, for one head.  In the pool [block][kv_head][KV_BLOCK][head_dim] those
//    rows are one contiguous run, and so they are in the buffer, so the workgroup's work is a straight copy of
//    rows * head_dim * elem_bytes bytes, at most 32 KB (bf16, head_dim 128).  Workgroups never touch each other's
//    bytes.  A 32k-token Mistral-7B slot is 131072 workgroups: the chip is full without a finer split.
//  - Every access is 16 bytes (a row is a whole number of 16-byte pieces, the buffer is 16-byte aligned).  A
//    thread has four loads in flight before its first store.
//  - In the last, partial block only the live rows move; rows at or above n, blocks beyond ceil(n / KV_BLOCK) and
//    blocks of other slots are neither read nor written.  A table entry that names no block of the pool is
//    skipped (pack may read the null block, as Engine::kv_read does; unpack never writes it).
// No LDS, no scratch, no atomics, no workspace.
#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ops.h"

namespace aios {

constexpr int KVP_THREADS = 256;

template <bool UNPACK>
__global__ __launch_bounds__(KVP_THREADS) void kv_snapshot_kernel(KvSnapArgs a) {
  const int nblk = (a.n_tokens + KV_BLOCK - 1) / KV_BLOCK;
  const int j = blockIdx.x % nblk, kvh = blockIdx.x / nblk;
  const int is_v = blockIdx.y, layer = blockIdx.z;
  const int phys = a.block_table[(size_t)a.slot * a.max_blocks + j];
  if (phys < 0 || phys > a.n_blocks || (UNPACK && phys == a.n_blocks)) return;  // (uniform over the workgroup)
  const int rows = min(KV_BLOCK, a.n_tokens - j * KV_BLOCK);
  const size_t rowb = (size_t)a.head_dim * a.elem_bytes;  // bytes of one row, a multiple of 16
  char* pool = (char*)pick_ptr(is_v == 0, a.k_cache, a.v_cache) + (size_t)(a.layer0 + layer) * a.layer_bytes +
               ((size_t)phys * a.n_kv_heads + kvh) * KV_BLOCK * rowb;
  char* buf = (char*)a.buf + ((((size_t)layer * 2 + is_v) * a.n_kv_heads + kvh) * a.n_tokens + (size_t)j * KV_BLOCK) * rowb;
  const uint4* __restrict__ src = (const uint4*)(UNPACK ? buf : pool);
  uint4* __restrict__ dst = (uint4*)(UNPACK ? pool : buf);
  const int pieces = (int)((size_t)rows * rowb / 16);  // <= KV_BLOCK * head_dim * 2 / 16
  constexpr int T = KVP_THREADS;
  int i = threadIdx.x;
  for (; i + 3 * T < pieces; i += 4 * T) {  // four loads in flight, then their stores (plain registers: no array)
    const uint4 r0 = src[i], r1 = src[i + T], r2 = src[i + 2 * T], r3 = src[i + 3 * T];
    dst[i] = r0;
    dst[i + T] = r1;
    dst[i + 2 * T] = r2;
    dst[i + 3 * T] = r3;
  }
  for (; i < pieces; i += T) dst[i] = src[i];
}

void launch_kv_snapshot(const KvSnapArgs& a, hipStream_t st) {
  if (!a.k_cache || !a.v_cache || !a.block_table || !a.buf) throw std::runtime_error("kv_snapshot: null argument");
  if (a.elem_bytes != 1 && a.elem_bytes != 2) throw std::runtime_error("kv_snapshot: element size must be 1 or 2");
  if (a.n_layers < 1 || a.layer0 < 0 || a.n_kv_heads < 1 || a.slot < 0 || a.max_blocks < 1 || a.n_blocks < 1 ||
      a.n_layers > 65535)
    throw std::runtime_error("kv_snapshot: bad shape");
  const int per16 = 16 / a.elem_bytes;  // elements of one 16-byte piece
  if (a.head_dim < per16 || a.head_dim % per16 || a.head_dim > 4096)
    throw std::runtime_error("kv_snapshot: head_dim " + std::to_string(a.head_dim) + " is not a multiple of " +
                             std::to_string(per16));
  if (a.n_tokens < 1 || a.n_tokens > (long long)a.max_blocks * KV_BLOCK)
    throw std::runtime_error("kv_snapshot: n_tokens out of range");
  if (((uintptr_t)a.buf | (uintptr_t)a.k_cache | (uintptr_t)a.v_cache | a.layer_bytes) & 15)
    throw std::runtime_error("kv_snapshot: pointers and the layer stride must be 16-byte aligned");
  // one layer's pool holds the n_blocks blocks and the null block
  if (a.layer_bytes < (size_t)(a.n_blocks + 1) * a.n_kv_heads * KV_BLOCK * a.head_dim * a.elem_bytes)
    throw std::runtime_error("kv_snapshot: layer stride smaller than the pool");
  const int nblk = (a.n_tokens + KV_BLOCK - 1) / KV_BLOCK;
  const dim3 grid((unsigned)nblk * a.n_kv_heads, 2, a.n_layers);
  if (a.unpack) hipLaunchKernelGGL(kv_snapshot_kernel<true>, grid, dim3(KVP_THREADS), 0, st, a);
  else hipLaunchKernelGGL(kv_snapshot_kernel<false>, grid, dim3(KVP_THREADS), 0, st, a);
}

}  // namespace aios
