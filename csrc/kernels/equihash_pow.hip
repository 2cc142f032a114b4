// Block hashes and target compare of (Equihash input, solution) pairs on the device: the host
// entry of eh_pow_check (csrc/kernels/equihash_pow.h). The miner's filter kernel itself is
// launched by the solver (EquihashGpuSolver::LaunchPow, equihash_solver.hip).
#include <hip/hip_runtime.h>

#include "kernels/equihash_pow.h"
#include "kernels/gpu_api.h"
#include "kernels/hip_util.h"

#include <cstring>
#include <stdexcept>

namespace bcp {
namespace gpu {

template <class P>
static void pow_check(const unsigned char* in140, const unsigned char* sols, size_t cnt, const unsigned char target_le[32],
                      std::vector<unsigned char>& hashes, std::vector<uint8_t>& pass) {
    DevBuf<uint32_t> d_in(cnt * 35), d_sol(cnt * P::SOLWORDS), d_hash(cnt * 8);
    DevBuf<uint8_t> d_pass(cnt);
    BCP_HIP_CHECK(hipMemcpy(d_in.p, in140, cnt * 140, hipMemcpyHostToDevice));
    BCP_HIP_CHECK(hipMemcpy(d_sol.p, sols, cnt * P::SOLW, hipMemcpyHostToDevice));
    bcpk::EhPowTarget t;
    memcpy(t.w, target_le, 32);
    hipLaunchKernelGGL((bcpk::eh_pow_check<P>), dim3((unsigned)cnt), dim3(64), 0, 0, d_in.p, d_sol.p, t, d_hash.p,
                       d_pass.p);
    BCP_HIP_CHECK(hipGetLastError());
    BCP_HIP_CHECK(hipMemcpy(hashes.data(), d_hash.p, cnt * 32, hipMemcpyDeviceToHost));
    BCP_HIP_CHECK(hipMemcpy(pass.data(), d_pass.p, cnt, hipMemcpyDeviceToHost));
}

void EquihashPowCheckBatch(unsigned n, unsigned k, const unsigned char* in140, const unsigned char* sols, size_t cnt,
                           const unsigned char target_le[32], std::vector<unsigned char>& hashes,
                           std::vector<uint8_t>& pass, int device) {
    if (cnt > 0x7fffffffu) throw std::invalid_argument("EquihashPowCheckBatch: too many pairs for one launch");
    DeviceScope scope(device);
    hashes.assign(cnt * 32, 0);
    pass.assign(cnt, 0);
    if (cnt == 0) return;
    if (n == 200 && k == 9) pow_check<bcpk::PowCfg<200, 9>>(in140, sols, cnt, target_le, hashes, pass);
    else if (n == 96 && k == 5) pow_check<bcpk::PowCfg<96, 5>>(in140, sols, cnt, target_le, hashes, pass);
    else if (n == 48 && k == 5) pow_check<bcpk::PowCfg<48, 5>>(in140, sols, cnt, target_le, hashes, pass);
    else throw std::invalid_argument("EquihashPowCheckBatch: unsupported (N,K); GPU supports (200,9),(96,5),(48,5)");
}

} // namespace gpu
} // namespace bcp
