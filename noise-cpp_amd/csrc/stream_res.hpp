// stream_res.hpp -- what the launchers cache under a caller's stream
// (internal; stream_res.hip).  One record per (device, stream) holds
//   - the grow-only scratch: the records path's classifier tables and segment
//     state (records_kernels.hip) and the uniform path's staging image of
//     unaligned batches (aead_kernels.hip) -- calls on one stream are ordered,
//     so they share it;
//   - the companion set of the records DAG (AuxStream), created on first use.
// records_scratch_release drops the record; a stream the engine created is
// closed through it (host_ctx.hpp, OwnedStream), a caller's stream by
// noise_gpu_scratch_release.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace noise_amd {

// chunks of the decrypt pipeline (records_kernels.hip, launch_classes); the
// companion set holds two events per chunk
#ifndef NOISE_SEG_CHUNKS
#define NOISE_SEG_CHUNKS 4
#endif
constexpr int kSegChunks = NOISE_SEG_CHUNKS;

// the scratch of (current device, stream), >= bytes.  It only grows: the
// smaller one is wiped and freed stream-ordered (dev_mem.hpp), after the
// launches that still use it
hipError_t records_scratch_get(void **p, size_t bytes, hipStream_t stream);
// zero the scratch of (current device, stream), stream-ordered; nothing to do
// for a stream that never took scratch
hipError_t records_scratch_wipe(hipStream_t stream);
// zero + free the scratch and destroy the companion set cached for (current
// device, stream); synchronises `stream`.  Call before destroying `stream`
hipError_t records_scratch_release(hipStream_t stream);

// Fork/join companions of a caller stream: three non-blocking streams and
// their events.  The records DAG has independent branches after the
// classifier (launch_classes); the short ones run on the companions while the
// segment kernel fills the GPU.
struct AuxStream {
  hipStream_t aux = nullptr;   // companion: small classes, generic, tails
  hipStream_t aux2 = nullptr;  // decrypt: per chunk, tag check + plaintext pass
  hipStream_t aux3 = nullptr;  // the whole-record classes of 2 .. 16 KiB
  // fork: classifier done; prep: k_seg_prep done; join: encrypt: the
  // companion branch done, decrypt: the tails' Poly1305 done; join2: the
  // companion done (decrypt); xdone: the last plaintext pass done; poly[c] /
  // fin[c]: chunk c's Poly1305 pass / tag check done
  hipEvent_t fork = nullptr, prep = nullptr, join = nullptr, join2 = nullptr, xdone = nullptr,
             big = nullptr;  // big: the whole-record classes done
  hipEvent_t poly[kSegChunks] = {}, fin[kSegChunks] = {};
};
// the companion set of (current device, stream), created on first use (a copy
// of the handles; they live until records_scratch_release)
hipError_t records_aux_get(AuxStream *out, hipStream_t stream);

}  // namespace noise_amd
