// A whole text against one automaton, split into strings ON THE DEVICE (include/mfa_hip.h, "text to batch"): one upload of the text,
// count, one read-back of the 32-byte info record, exact allocation, write, the plain match call, results back -- on one device, on
// its default stream.  The only file of the host mirror that calls the HIP runtime itself (device memory and copies): it does not
// include diploma_api.h, whose `enum MemoryAction { open, close }` clashes with the system headers the runtime's header pulls in.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mfa_hip.h"

namespace {

struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess ? MFA_OK : MFA_ERR_NOMEM; }
};

}  // namespace

// results: one 0/1/2 byte per string, as mfa_match_batch leaves them.  *longest: the longest string of the text in bytes; when it passes
// `longest_allowed` the results are NOT valid (they are empty) and the caller takes another way.  Returns MFA_OK or an MFA_ERR_* code.
int diploma_match_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, uint32_t mode, const char* stop, uint64_t longest_allowed,
                                 int device, std::vector<uint8_t>& results, uint64_t* longest) {
    results.clear();
    *longest = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return MFA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return MFA_ERR_HIP;
    size_t work_bytes = 0;
    int rc = mfa_split_workspace_bytes(n, &work_bytes);
    if (rc != MFA_OK) return rc;
    DeviceBuffer d_text, d_work, d_info, d_bytes, d_offsets, d_results;
    const size_t room = (n + 15) / 16 * 16;                      // the read rule: whole 16-byte blocks
    if ((rc = d_text.alloc(room)) != MFA_OK || (rc = d_work.alloc(work_bytes)) != MFA_OK || (rc = d_info.alloc(sizeof(mfa_split_info))) != MFA_OK) return rc;
    if (n && hipMemcpy(d_text.p, text, n, hipMemcpyHostToDevice) != hipSuccess) return MFA_ERR_HIP;
    rc = mfa_split_text_count(n ? (const uint8_t*)d_text.p : nullptr, n, mode, stop, d_work.p, (mfa_split_info*)d_info.p, device, nullptr);
    if (rc != MFA_OK) return rc;
    mfa_split_info info;
    if (hipMemcpy(&info, d_info.p, sizeof info, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;      // the one read-back of the info
    const uint64_t capacity = (info.n_bytes + 15) / 16 * 16;     // what the read rule of mfa_match_batch asks for
    // the results travel back with the info record behind them, which by then holds max_string_bytes
    if ((rc = d_bytes.alloc(capacity)) != MFA_OK || (rc = d_offsets.alloc((info.n_strings + 1) * 8)) != MFA_OK ||
        (rc = d_results.alloc(info.n_strings + sizeof info)) != MFA_OK) return rc;
    rc = mfa_split_text_write(n ? (const uint8_t*)d_text.p : nullptr, n, mode, d_work.p, (mfa_split_info*)d_info.p, (uint8_t*)d_bytes.p, capacity,
                              (uint64_t*)d_offsets.p, info.n_strings, device, nullptr);
    if (rc != MFA_OK) return rc;
    if (info.n_strings) {
        rc = mfa_match_batch(img, (const uint8_t*)d_bytes.p, (const uint64_t*)d_offsets.p, info.n_strings, (uint8_t*)d_results.p, device, nullptr);
        if (rc != MFA_OK) return rc;
    }
    if (hipMemcpyAsync((uint8_t*)d_results.p + info.n_strings, d_info.p, sizeof info, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return MFA_ERR_HIP;
    std::vector<uint8_t> back(info.n_strings + sizeof info);
    if (hipMemcpy(back.data(), d_results.p, back.size(), hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;
    memcpy(&info, back.data() + info.n_strings, sizeof info);
    *longest = info.max_string_bytes;
    if (info.overflow) return MFA_ERR_INVALID_ARG;               // (exact room was given: cannot happen)
    if (info.max_string_bytes > longest_allowed) return MFA_OK;  // the caller's other way
    back.resize(info.n_strings);
    results.swap(back);
    return MFA_OK;
}
