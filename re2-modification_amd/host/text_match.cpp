// A whole text against one automaton, split into strings ON THE DEVICE (include/mfa_hip.h, "text to batch"): one upload of the text,
// count, one read-back of the 32-byte info record, exact allocation, write, the plain match call, results back -- on one device, on
// its default stream.  And the same with the way out on the device too ("batch to text"): the strings that matched come back as a text,
// no offsets and no result bytes.  The only file of the host mirror that calls the HIP runtime itself (device memory and copies): it does not
// include diploma_api.h, whose `enum MemoryAction { open, close }` clashes with the system headers the runtime's header pulls in.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <string>
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

// The strings of the text that the automaton accepts (rejects, with `invert`), each with a 0x0a behind it, in `out`: split, matched and
// selected on the device; what travels back is the 32-byte info record of the selection (with the splitter's behind it) and the kept
// bytes.  *longest as above: when it passes `longest_allowed`, `out` is empty and the caller takes another way.  *n_unanswered: strings
// the match call answered neither 0 nor 1; they are not kept.
int diploma_select_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, uint32_t mode, const char* stop, uint64_t longest_allowed,
                                  int device, bool invert, std::string& out, uint64_t* n_unanswered, uint64_t* longest) {
    out.clear();
    *longest = 0;
    *n_unanswered = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return MFA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return MFA_ERR_HIP;
    size_t work_bytes = 0;
    int rc = mfa_split_workspace_bytes(n, &work_bytes);
    if (rc != MFA_OK) return rc;
    struct Infos { mfa_select_info select; mfa_split_info split; } infos;      // one record behind the other on the device: one read-back
    DeviceBuffer d_text, d_work, d_infos, d_bytes, d_offsets, d_results, d_select_work, d_out, d_out_offsets;
    const size_t room = (n + 15) / 16 * 16;                      // the read rule: whole 16-byte blocks
    if ((rc = d_text.alloc(room)) != MFA_OK || (rc = d_work.alloc(work_bytes)) != MFA_OK || (rc = d_infos.alloc(sizeof infos)) != MFA_OK) return rc;
    mfa_select_info* const d_select_info = (mfa_select_info*)d_infos.p;
    mfa_split_info* const d_split_info = (mfa_split_info*)((uint8_t*)d_infos.p + sizeof(mfa_select_info));
    if (n && hipMemcpy(d_text.p, text, n, hipMemcpyHostToDevice) != hipSuccess) return MFA_ERR_HIP;      // the one upload
    rc = mfa_split_text_count(n ? (const uint8_t*)d_text.p : nullptr, n, mode, stop, d_work.p, d_split_info, device, nullptr);
    if (rc != MFA_OK) return rc;
    mfa_split_info split;
    if (hipMemcpy(&split, d_split_info, sizeof split, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;
    const uint64_t n_strings = split.n_strings, capacity = (split.n_bytes + 15) / 16 * 16;
    size_t select_work_bytes = 0;
    if ((rc = mfa_select_workspace_bytes(n_strings, &select_work_bytes)) != MFA_OK) return rc;
    if ((rc = d_bytes.alloc(capacity)) != MFA_OK || (rc = d_offsets.alloc((n_strings + 1) * 8)) != MFA_OK || (rc = d_results.alloc(n_strings)) != MFA_OK ||
        (rc = d_select_work.alloc(select_work_bytes)) != MFA_OK) return rc;
    rc = mfa_split_text_write(n ? (const uint8_t*)d_text.p : nullptr, n, mode, d_work.p, d_split_info, (uint8_t*)d_bytes.p, capacity,
                              (uint64_t*)d_offsets.p, n_strings, device, nullptr);
    if (rc != MFA_OK) return rc;
    if (n_strings) {
        rc = mfa_match_batch(img, (const uint8_t*)d_bytes.p, (const uint64_t*)d_offsets.p, n_strings, (uint8_t*)d_results.p, device, nullptr);
        if (rc != MFA_OK) return rc;
    }
    const uint32_t flags = MFA_SELECT_NEWLINE | (invert ? MFA_SELECT_INVERT : 0u);
    rc = mfa_select_count((const uint8_t*)d_results.p, (const uint64_t*)d_offsets.p, n_strings, flags, d_select_work.p, d_select_info, device, nullptr);
    if (rc != MFA_OK) return rc;
    if (hipMemcpy(&infos, d_infos.p, sizeof infos, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;      // the one read-back of the info
    *longest = infos.split.max_string_bytes;
    if (infos.split.overflow) return MFA_ERR_INVALID_ARG;        // (exact room was given: cannot happen)
    if (infos.split.max_string_bytes > longest_allowed) return MFA_OK;      // the caller's other way
    *n_unanswered = infos.select.n_unanswered;
    if ((rc = d_out.alloc(infos.select.n_bytes)) != MFA_OK || (rc = d_out_offsets.alloc((infos.select.n_selected + 1) * 8)) != MFA_OK) return rc;
    rc = mfa_select_write((const uint8_t*)d_bytes.p, (const uint64_t*)d_offsets.p, (const uint8_t*)d_results.p, n_strings, flags, d_select_work.p,
                          d_select_info, (uint8_t*)d_out.p, infos.select.n_bytes, (uint64_t*)d_out_offsets.p, nullptr, infos.select.n_selected, device, nullptr);
    if (rc != MFA_OK) return rc;
    out.resize(infos.select.n_bytes);
    if (infos.select.n_bytes && hipMemcpy(&out[0], d_out.p, infos.select.n_bytes, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;      // exactly n_bytes
    return MFA_OK;
}

// Search inside the lines of the text (include/mfa_hip.h, "search inside lines"): split, searched and selected on the device.  `out` gets
// the lines that hold a match (`invert`: that hold none), or with `only_matching` the leftmost-longest match of every line that has one,
// each with a 0x0a behind it.  only_matching selects from the spans themselves: they are the offsets of 2n strings over the same bytes,
// string 2k line k's match, and the span results keep exactly those.  What travels back: the splitter's info record, the selection's,
// and the kept bytes.  *n_unanswered: lines beyond MFA_MAX_STRING_BYTES, which the search does not read; they are not kept.
int diploma_search_text_on_device(mfa_image_t* img, const uint8_t* text, size_t n, int device, bool invert, bool only_matching, std::string& out,
                                  uint64_t* n_unanswered) {
    out.clear();
    *n_unanswered = 0;
    if (invert && only_matching) return MFA_ERR_INVALID_ARG;
    uint32_t sets1 = 0, sets2 = 0;
    int rc = mfa_image_search_info(img, &sets1, &sets2);           // an image the search refuses: before the device is touched
    if (rc != MFA_OK) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return MFA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return MFA_ERR_HIP;
    size_t work_bytes = 0;
    if ((rc = mfa_split_workspace_bytes(n, &work_bytes)) != MFA_OK) return rc;
    DeviceBuffer d_text, d_work, d_split_info, d_select_info, d_bytes, d_offsets, d_results, d_spans, d_span_results, d_select_work, d_out, d_out_offsets;
    const size_t room = (n + 15) / 16 * 16;                      // the read rule: whole 16-byte blocks
    if ((rc = d_text.alloc(room)) != MFA_OK || (rc = d_work.alloc(work_bytes)) != MFA_OK || (rc = d_split_info.alloc(sizeof(mfa_split_info))) != MFA_OK ||
        (rc = d_select_info.alloc(sizeof(mfa_select_info))) != MFA_OK) return rc;
    if (n && hipMemcpy(d_text.p, text, n, hipMemcpyHostToDevice) != hipSuccess) return MFA_ERR_HIP;      // the one upload
    const uint8_t* const src = n ? (const uint8_t*)d_text.p : nullptr;
    rc = mfa_split_text_count(src, n, MFA_SPLIT_LINES, nullptr, d_work.p, (mfa_split_info*)d_split_info.p, device, nullptr);
    if (rc != MFA_OK) return rc;
    mfa_split_info split;
    if (hipMemcpy(&split, d_split_info.p, sizeof split, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;
    const uint64_t n_lines = split.n_strings, capacity = (split.n_bytes + 15) / 16 * 16;
    const uint64_t n_select = only_matching ? 2u * n_lines : n_lines;
    size_t select_work_bytes = 0;
    if ((rc = mfa_select_workspace_bytes(n_select, &select_work_bytes)) != MFA_OK) return rc;
    if ((rc = d_bytes.alloc(capacity)) != MFA_OK || (rc = d_offsets.alloc((n_lines + 1) * 8)) != MFA_OK || (rc = d_results.alloc(n_lines)) != MFA_OK ||
        (rc = d_select_work.alloc(select_work_bytes)) != MFA_OK) return rc;
    if (only_matching && ((rc = d_spans.alloc((2u * n_lines + 1u) * 8)) != MFA_OK || (rc = d_span_results.alloc(2u * n_lines)) != MFA_OK)) return rc;
    rc = mfa_split_text_write(src, n, MFA_SPLIT_LINES, d_work.p, (mfa_split_info*)d_split_info.p, (uint8_t*)d_bytes.p, capacity, (uint64_t*)d_offsets.p,
                              n_lines, device, nullptr);
    if (rc != MFA_OK) return rc;
    rc = mfa_search_batch(img, (const uint8_t*)d_bytes.p, (const uint64_t*)d_offsets.p, n_lines, (uint8_t*)d_results.p,
                          only_matching ? (uint64_t*)d_spans.p : nullptr, only_matching ? (uint8_t*)d_span_results.p : nullptr, device, nullptr);
    if (rc != MFA_OK) return rc;
    const uint32_t flags = MFA_SELECT_NEWLINE | (invert ? MFA_SELECT_INVERT : 0u);
    const uint64_t* const sel_offsets = only_matching ? (const uint64_t*)d_spans.p : (const uint64_t*)d_offsets.p;
    const uint8_t* const sel_results = only_matching ? (const uint8_t*)d_span_results.p : (const uint8_t*)d_results.p;
    rc = mfa_select_count(sel_results, sel_offsets, n_select, flags, d_select_work.p, (mfa_select_info*)d_select_info.p, device, nullptr);
    if (rc != MFA_OK) return rc;
    mfa_select_info sel;
    if (hipMemcpy(&sel, d_select_info.p, sizeof sel, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;      // the one read-back of the selection
    *n_unanswered = sel.n_unanswered;
    if ((rc = d_out.alloc(sel.n_bytes)) != MFA_OK || (rc = d_out_offsets.alloc((sel.n_selected + 1) * 8)) != MFA_OK) return rc;
    rc = mfa_select_write((const uint8_t*)d_bytes.p, sel_offsets, sel_results, n_select, flags, d_select_work.p, (mfa_select_info*)d_select_info.p,
                          (uint8_t*)d_out.p, sel.n_bytes, (uint64_t*)d_out_offsets.p, nullptr, sel.n_selected, device, nullptr);
    if (rc != MFA_OK) return rc;
    out.resize(sel.n_bytes);
    if (sel.n_bytes && hipMemcpy(&out[0], d_out.p, sel.n_bytes, hipMemcpyDeviceToHost) != hipSuccess) return MFA_ERR_HIP;      // exactly n_bytes
    return MFA_OK;
}
