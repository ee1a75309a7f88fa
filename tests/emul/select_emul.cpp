// TEST INFRASTRUCTURE ONLY: the host-compilable core of the selection (csrc/select_core.h: the kept rule, the workspace, the tile geometry,
// the searches, a chunk's way from aligned source blocks through the staging area to the destination) run in the order of the kernels of
// csrc/select.hip: the count pass block by block, the scan over the blocks' totals, the place pass block by block, the gather pass tile
// by tile through a staging area of the tile's size -- the workgroup's searches round by round, the fill lane by lane (by runs of chunks or
// by strings, as the kernel chooses), then the stores chunk by chunk.
//   select_emul CASES.bin > OUT.bin
//       CASES.bin: u32 count, then per case  u32 flags, u32 src_shift, u32 dst_shift, u32 with_indices, u64 max_selected,
//                  u64 bytes_capacity, u64 n, offsets[0..n] as u64, n result bytes, offsets[n] - offsets[0] bytes of strings.
//                  src_shift, dst_shift: d_bytes & 15 and d_out_bytes & 15.
//       OUT.bin:   per case  the 32 bytes of mfa_select_info, u64 v = min(n_selected, max_selected), out_offsets[0..v] as u64,
//                  out_indices[0..v) as u64 (with_indices only), then min(out_offsets[v], bytes_capacity) bytes.
//       The strings lie in exactly the aligned 16-byte blocks they touch, the three outputs in exactly their capacities (d_out_bytes ends
//       where its allocation ends; the dst_shift bytes in front of it are guard bytes the harness checks), so that a host sanitizer sees
//       every access beyond them.
#include "emul_common.h"
#include "mfa_hip.h"
#include "select_core.h"

using namespace mfa;

struct Case {
    uint32_t flags, src_shift, dst_shift, with_indices;
    uint64_t max_selected, capacity, n;
    std::vector<uint64_t> off;
    const uint8_t* results;
    const uint8_t* data;
};

static void fail(const char* what) { fprintf(stderr, "%s\n", what); exit(5); }

static void* exact(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1)) fail("out of memory");
    return p;
}

static void run_case(const Case& c, FILE* out) {
    // the source: d_bytes & 15 == src_shift, readable in the aligned blocks that [d_bytes + off[0], d_bytes + off[n]) touches and nowhere else
    const uint64_t first = (c.src_shift + c.off[0]) & ~(uint64_t)15, last = (c.src_shift + c.off[c.n] + 15u) & ~(uint64_t)15;
    const uint64_t room = c.off[c.n] > c.off[0] ? last - first : 0;
    uint8_t* const blocks = (uint8_t*)exact(room);
    memset(blocks, 0xa5, room);
    const uint8_t* const d_bytes = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(blocks) - first + c.src_shift);
    if (room) memcpy(blocks + (c.src_shift + c.off[0] - first), c.data, c.off[c.n] - c.off[0]);

    const uint64_t nb = select_blocks(c.n);
    uint8_t* const work = (uint8_t*)exact(select_workspace_bytes(c.n));
    SelectTotals* totals = reinterpret_cast<SelectTotals*>(work);
    SelectPrefix* prefix = reinterpret_cast<SelectPrefix*>(work + select_prefix_at(nb));
    uint16_t* list = reinterpret_cast<uint16_t*>(work + select_list_at(nb));
    mfa_select_info info{};

    // count
    for (uint64_t b = 0; b < nb; b++) {
        SelectTotals t{0, 0, 0};
        for (uint32_t i = 0; i < kSelectBlock && b * kSelectBlock + i < c.n; i++) {
            const uint64_t k = b * kSelectBlock + i;
            const bool kept = select_kept(c.results[k], c.flags);
            if (kept) list[b * kSelectBlock + t.kept++] = (uint16_t)i;
            t.unanswered += select_unanswered(c.results[k]) ? 1u : 0u;
            t.bytes += select_out_len(kept, c.off[k + 1] - c.off[k], c.flags);
        }
        totals[b] = t;
    }
    // scan
    {
        SelectPrefix at{0, 0};
        for (uint64_t b = 0; b < nb; b++) {
            prefix[b] = at;
            at.bytes += totals[b].bytes; at.kept += totals[b].kept; info.n_unanswered += totals[b].unanswered;
        }
        prefix[nb] = at;
        info.n_selected = at.kept;
        info.n_bytes = at.bytes;
    }
    // place
    uint64_t* const out_offsets = (uint64_t*)exact((c.max_selected + 1) * 8);
    uint64_t* const out_indices = c.with_indices ? (uint64_t*)exact(c.max_selected * 8) : nullptr;
    memset(out_offsets, 0x5a, (c.max_selected + 1) * 8);
    if (out_indices) memset(out_indices, 0x5a, c.max_selected * 8);
    if (info.n_selected <= c.max_selected) out_offsets[info.n_selected] = info.n_bytes;
    info.overflow = (info.n_selected > c.max_selected || info.n_bytes > c.capacity) ? 1u : 0u;
    for (uint64_t b = 0; b < (nb ? nb : 1); b++) {
        uint64_t rank = prefix[b].kept, at = prefix[b].bytes;
        for (uint32_t i = 0; i < kSelectBlock && b * kSelectBlock + i < c.n; i++) {
            const uint64_t k = b * kSelectBlock + i;
            if (!select_kept(c.results[k], c.flags)) continue;
            if (rank <= c.max_selected) out_offsets[rank] = at;
            if (out_indices && rank < c.max_selected) out_indices[rank] = k;
            rank++;
            at += select_out_len(true, c.off[k + 1] - c.off[k], c.flags);
        }
        if (nb && (rank != prefix[b + 1].kept || at != prefix[b + 1].bytes)) fail("the passes disagree on a block");
    }
    // gather
    uint8_t* const dst_alloc = (uint8_t*)exact(c.dst_shift + c.capacity);      // d_out_bytes ends where the allocation ends
    memset(dst_alloc, 0x5a, c.dst_shift + c.capacity);
    uint8_t* const d_out = dst_alloc + c.dst_shift;
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    if (skew != c.dst_shift) fail("the destination is not where the case wants it");
    const uint64_t v = select_min(info.n_selected, c.max_selected);
    if (nb && c.capacity) {
        uint8_t* const s_out = (uint8_t*)exact(kSelectTileBytes);
        const uint64_t tiles = select_tiles(select_min(c.capacity, kSelectMaxCapacity), skew);
        const uint64_t limit = select_min(out_offsets[v], c.capacity);
        const SelectSource src{d_bytes, c.off.data(), out_offsets, out_indices, prefix, list, (c.flags & kSelectNewline) ? 1u : 0u};
        for (uint64_t tile = 0; tile < tiles; tile++) {
            const SelectTile t = select_tile(tile, skew, limit);
            if (t.end <= t.begin) continue;
            memset(s_out, 0xc3, kSelectTileBytes);
            // the four searches of the workgroup, round by round, each against the plain binary search
            SelectReach reach{0, 0, 0, 0};
            for (uint32_t which = 0; which < 4u; which++) {
                const SelectSearch q = select_reach_search(which, reach, prefix, nb, out_offsets, v, t.begin - skew, t.end - skew - 1u);
                if (q.lo > q.hi || q.a[q.lo * q.stride] > q.x) fail("a search begins outside its range");
                uint64_t lo = q.lo, hi = q.hi;
                for (uint32_t rounds = 0; lo < hi; rounds++) {
                    if (rounds > 8u) fail("a search does not end");
                    const uint64_t step = select_search_step(lo, hi);
                    uint32_t count = 0;
                    for (uint32_t tid = 0; tid < kSelectThreads; tid++) {
                        const bool ok = select_search_probe(q.a, q.stride, lo, hi, step, tid, q.x);
                        if (ok && count != tid) fail("the probes of a round are not a run of lanes");
                        count += ok ? 1u : 0u;
                    }
                    select_search_narrow(lo, hi, step, count);
                }
                if (lo != select_last_le(q.a, q.stride, q.lo, q.hi, q.x)) fail("the workgroup's search and the binary search differ");
                select_reach_set(which, reach, lo);
            }
            if (reach.r_lo != select_last_le(out_offsets, 1u, 0u, v, t.begin - skew) || reach.r_hi != select_last_le(out_offsets, 1u, 0u, v, t.end - skew - 1u))
                fail("the ranks of a tile are not those of a search in all offsets");
            if (reach.r_hi >= v || reach.b_hi >= nb) fail("a search left its range");
            uint8_t* const dst_line = d_out - skew + t.line0;
            uint64_t covered = 0;
            for (uint32_t tid = 0; tid < kSelectThreads; tid++) {        // fill: by strings or by runs of chunks, as the kernel chooses
                if (select_by_strings(reach)) {
                    select_fill_strings(src, s_out, t, skew, reach, tid);
                } else {
                    const SelectChunk head = select_chunk(t, tid * kSelectPerLane), tail = select_chunk(t, tid * kSelectPerLane + kSelectPerLane - 1u);
                    select_fill_run(src, s_out, t, head.begin, tail.end > head.begin ? tail.end : head.begin, skew, reach);
                }
            }
            for (uint32_t tid = 0; tid < kSelectThreads; tid++)          // behind the barrier: the stores
                for (uint32_t i = 0; i < kSelectPerLane; i++) {
                    const SelectChunk ch = select_chunk(t, i * kSelectThreads + tid);
                    if (ch.end <= ch.begin) continue;
                    if (ch.end - ch.begin > 16u || ch.begin < t.begin || ch.end > t.end) fail("a chunk outside its tile");
                    if (ch.end - ch.begin == 16u && ((reinterpret_cast<uintptr_t>(dst_line) + (ch.begin - t.line0)) & 15u)) fail("a vector store off its line");
                    if (ch.end - ch.begin != 16u && ch.begin != skew && ch.end != limit + skew) fail("a partial chunk inside the output");
                    select_store_chunk(s_out, dst_line, t, ch);
                    covered += ch.end - ch.begin;
                }
            if (covered != t.end - t.begin) fail("the chunks do not cover their tile");
        }
        free(s_out);
    }
    for (uint32_t i = 0; i < c.dst_shift; i++)
        if (dst_alloc[i] != 0x5a) fail("a byte in front of d_out_bytes was written");

    fwrite(&info, sizeof info, 1, out);
    fwrite(&v, 8, 1, out);
    fwrite(out_offsets, 8, v + 1, out);
    if (out_indices) fwrite(out_indices, 8, v, out);
    fwrite(d_out, 1, select_min(out_offsets[v], c.capacity), out);
    free(dst_alloc); free(out_offsets); free(out_indices); free(work); free(blocks);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: select_emul CASES.bin > OUT.bin\n"); return 2; }
    const std::vector<uint8_t> file = emul::slurp(argv[1]);
    const uint8_t* p = file.data();
    uint32_t count;
    memcpy(&count, p, 4); p += 4;
    for (uint32_t k = 0; k < count; k++) {
        Case c;
        memcpy(&c.flags, p, 4); memcpy(&c.src_shift, p + 4, 4); memcpy(&c.dst_shift, p + 8, 4); memcpy(&c.with_indices, p + 12, 4);
        memcpy(&c.max_selected, p + 16, 8); memcpy(&c.capacity, p + 24, 8); memcpy(&c.n, p + 32, 8);
        p += 40;
        if ((c.flags & ~3u) || c.src_shift > 15u || c.dst_shift > 15u || c.n >= kSelectMaxStrings) { fprintf(stderr, "case %u: refused\n", k); return 3; }
        c.off.resize(c.n + 1);
        memcpy(c.off.data(), p, (c.n + 1) * 8); p += (c.n + 1) * 8;
        c.results = p; p += c.n;
        c.data = p; p += c.off[c.n] - c.off[0];
        run_case(c, stdout);
    }
    if (p != file.data() + file.size()) { fprintf(stderr, "bytes behind the last case\n"); return 3; }
    return 0;
}
