// wingest.hpp -- host-side launchers of k_wingest.hip (the worker's message
// ingestion on the device; used by wingest_gpu.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nt {

constexpr uint64_t kWmsgSlack = 64;  // readable bytes before / after the wire bytes (as in k_ingest.hip)

// One chunk of n messages.
struct WmsgBufs {
  const uint8_t* wire;   // kWmsgSlack bytes, the chunk's wire bytes, kWmsgSlack bytes
  uint64_t wire_bytes;   // the slack in front plus the wire bytes: no message reaches past it
  const uint64_t* moff;  // message i = wire[moff[i] .. moff[i] + mlen[i]); moff[i] >= kWmsgSlack
  const uint64_t* mlen;
  uint64_t n;
  uint4* plan;           // k_wmsg_walk: [n][4], the receipt with a batch's digest still zero
  uint64_t* hlen;        // k_wmsg_walk: [n], the length the SHA-512 launch hashes (an OK batch: mlen[i], else 0)
  uint8_t* code;         // k_wmsg_walk: [n]
  const uint8_t* sha;    // the SHA-512 launch: [n][32]
  uint4* rec;            // k_wmsg_receipt: [n][4] (ntcrypto.h nt_worker_receipt)
};
hipError_t launch_wmsg_walk(const WmsgBufs& b, hipStream_t s);
// after launch_wmsg_walk and the SHA-512 launch on the same stream
hipError_t launch_wmsg_receipt(const WmsgBufs& b, hipStream_t s);

}  // namespace nt
