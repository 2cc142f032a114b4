// The relay context of a device, shared by the relay-path translation units (relay.hip,
// wallet_match.hip): one stream and grow-only pinned/device staging; calls on one device are
// serialised by its mutex.
#pragma once
#include "kernels/hip_util.h"

#include <mutex>

namespace bcp {
namespace gpu {

struct RelayCtx {
    std::mutex m;
    hipStream_t s = nullptr;
    LaneState st; // staging slots only (the stream above is the one used)
};
inline RelayCtx& Ctx(int device) {
    static RelayCtx ctx[64];
    if (device < 0 || device >= 64) throw std::runtime_error("relay GPU context: device index out of range");
    return ctx[device];
}
inline std::unique_lock<std::mutex> Lock(RelayCtx& c) {
    std::unique_lock<std::mutex> l(c.m);
    if (!c.s) BCP_HIP_CHECK(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    return l;
}

} // namespace gpu
} // namespace bcp
