/* C-ABI of the MI355X match path (libmfa_hip.so).
 *
 * This is the drop-in boundary for the reference's match loop: everything the
 * reference does between "automaton compiled" and "0/1 per string" --
 *     bool MFA::match(string)              reference automata.h:69, mfa.cpp:215-236
 *     bool Automata::match(const string&)  reference automata.h:42, automata.cpp:177-210
 *     the per-string loops that call them  reference matchers/match.cpp:21-31,
 *                                          matchers/match_mfa.cpp:28-36,72-80
 * -- for a whole batch of strings at once, on the GPU.  The reference has no FFI
 * of its own (it is one C++ process); these are the entry points its
 * `Automata`/`MFA` classes bind when the match loop is moved to the device (the
 * binding is shown in INTEGRATION.md, our own host mirror of those classes lives in
 * re2-modification_amd/host/).
 *
 * Plain C types only: pointers and sizes.  No exceptions cross this boundary;
 * every function returns 0 (MFA_OK) or a negative MFA_ERR_* code.  The caller owns
 * every buffer it passes.  Functions are re-entrant per (image, device, stream):
 * every launch takes its own workspace (ticket counter, scratch, region table,
 * events) from a per-image pool, so one image may be used from several host threads
 * and on several streams at the same time; launches on one stream run in stream order.
 *
 * There is NO CPU fallback: without a usable HIP device the match entry points
 * return MFA_ERR_NO_DEVICE.
 */
#ifndef MFA_HIP_H
#define MFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "mfa_image_format.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_OK                 0
#define MFA_ERR_INVALID_ARG   -1  /* NULL pointer, bad size                                            */
#define MFA_ERR_BAD_BLOB      -2  /* blob fails the format checks of mfa_image_format.h                */
#define MFA_ERR_UNSUPPORTED   -3  /* well-formed automaton outside the kernels' limits (see below)     */
#define MFA_ERR_NO_DEVICE     -4  /* no HIP device / device index out of range                         */
#define MFA_ERR_HIP           -5  /* a HIP runtime call failed; mfa_last_hip_error() has the code       */
#define MFA_ERR_NOMEM         -6
#define MFA_ERR_TOO_LONG      -7  /* a string is longer than MFA_MAX_STRING_BYTES                       */
#define MFA_ERR_JIT           -8  /* compiling a specialised kernel failed (the table-driven walk still works) */

/* limits of the device kernels (violations -> MFA_ERR_UNSUPPORTED at image creation) */
#define MFA_MAX_NODES        1024u     /* MFA kind: nodes (any out-degree)                 */
#define MFA_MAX_KERNEL_CELLS 9u        /* MFA kind: distinct memory cells ("1".."9", mfa.cpp:148) */
#define MFA_MAX_DFA_STATES   (1u << 20) /* NFA kind: reachable state sets after tabulation; beyond them the image is a set-walk image (below) */
#define MFA_MAX_STRING_BYTES 0x00ffffffu /* 16 MiB - 1 per string                          */
/* NFA kind, EVERY image, tabulated or not: a cycle of epsilon edges among the nodes that can be reached from `start` over edges of any
 * kind is MFA_ERR_UNSUPPORTED.  The reference's evaluateState (automata.cpp:98-117) marks a node only after its scan and does not return
 * once it enters such a cycle; the check is made on the graph, so it also refuses a cycle that no input would make it enter. */

typedef struct mfa_image mfa_image_t;

typedef struct mfa_image_info {
    uint32_t kind;         /* MFA_KIND_NFA / MFA_KIND_MFA                                   */
    uint32_t is_reversed;
    uint32_t n_nodes, n_edges, n_cells;
    uint32_t dfa_states;   /* NFA kind: number of tabulated state sets (incl. the dead set); 0: a set-walk image */
    uint32_t byte_classes; /* NFA kind: number of input byte classes                        */
    uint32_t last_kernel;  /* MFA_KERNEL_*: which kernel the last match call on this image launched */
} mfa_image_info;

#define MFA_KERNEL_NONE        0u
#define MFA_KERNEL_WALK        1u /* walk_kernel: table-driven memory-automaton walk over a list of live states (any automaton, no compiler) */
#define MFA_KERNEL_SPECIALISED 2u /* mfa_jit_kernel: the walk generated for one automaton, one slot per node in VGPRs */
#define MFA_KERNEL_TABLE       3u /* dfa_walk_kernel: tabulated memory-less automaton                    */
#define MFA_KERNEL_NODESET     4u /* nfa_set_kernel, nfa_set_resume_kernel, nfa_set_wave_kernel: memory-less automaton beyond the tabulation limit, walked as a set of live nodes */
/* what a call that is no match call leaves in last_kernel; numbered on from the match kernels above */
#define MFA_KERNEL_SEARCH      (MFA_KERNEL_NODESET + 1u) /* = 5: search_pass1_*_kernel, search_pass2_kernel -- mfa_search_batch, the search inside lines */

/* Build an image from a blob (include/mfa_image_format.h).  Host-only work: parse,
 * check the structural invariants the kernels rely on, and for MFA_KIND_NFA tabulate
 * the reference's step function (automata.cpp:98-128) into a transition table.
 * Needs no GPU.  Replaces: holding an `Automata*` / `MFA*` (automata.h:18-84).
 *
 * Set-walk images.  A memory-less automaton whose reachable state sets pass MFA_MAX_DFA_STATES (or MFA_DFA_STATE_LIMIT=n, a lower limit
 * from the environment) is not tabulated: the image keeps the automaton's nodes, dfa_states is 0, and the match calls walk the SET of
 * live nodes, one string per lane, with the reference's own step per byte (last_kernel: MFA_KERNEL_NODESET).  MFA_NFA_SETWALK=1 makes
 * every memory-less image such an image without tabulating, MFA_NFA_SETWALK=0 none (beyond the limit: MFA_ERR_UNSUPPORTED, as it used
 * to be); both knobs are read here, at image creation.  Limits of such an image (MFA_ERR_UNSUPPORTED at creation): at most 2048 nodes and
 * 255 byte classes, no cycle of epsilon edges among the nodes reachable from the start (the reference's evaluateState would not return),
 * and, for an image of up to 256 nodes, epsilon chains of at most 49 nodes.  Wave images: up to 256 nodes a lane holds the set and walks
 * a string (nfa_set_kernel); an image of 257 to 2048 nodes is a WAVE image: one string per wave, the set across its 64 lanes
 * (nfa_set_wave_kernel; last_kernel is MFA_KERNEL_NODESET all the same), epsilon chains of any length.  What is said below about long
 * strings applies to a wave image too (mfa_match_batch, _host, _regions, its segment of a mixed object, and the wide resume call), with
 * a WAVE per chunk where a lane image has a lane: the same scheme, the same knobs and the same report in mfa_last_set_split; only the
 * chunk minimum (1024 bytes) and the arena differ -- a chunk takes 816 bytes of it and at most 32768 chunks are planned for, about 55 MB
 * per overlapping launch.  Its strings in pieces have a record and a call of their own: mfa_match_batch_resume_set refuses it,
 * mfa_match_batch_resume_set_wide (further down) takes it.  MFA_SET_WAVE=1, read here too, makes EVERY set-walk
 * image a wave image, the narrow ones as well: a knob for measurements and tests, never the default (the lane kernel is many times
 * faster where it applies).  Strings in pieces: its state between two bytes is a set of nodes, not one 32-bit number, so
 * mfa_match_batch_resume and _resume_host answer MFA_ERR_UNSUPPORTED before the device is touched, and mfa_match_batch_resume_set (below)
 * is the call that carries such a set from piece to piece (for a wave image: mfa_match_batch_resume_set_wide;
 * mfa_image_resume_state_bytes tells which).  Long strings: a string of MFA_DFA_SPLIT_MIN bytes or more (default 65536) is
 * cut into chunks inside the same call, as for a table in L2 (mfa_match_batch below has the scheme): every chunk is walked from ONE node
 * set by a lane of its own -- the first chunk from the true set, the others from a guess, the set reached over the MFA_SET_SPLIT_LOOKBACK
 * bytes (default 64) in front of the chunk from {start} or, if that walk dies, from a "home" set chosen per image -- then
 * MFA_SET_SPLIT_ROUNDS launches (default 3, at most 8; fixed when the call is enqueued) walk again every chunk that was not started from
 * what its predecessor ended in, and a last step follows each string's chunks from its true set and walks serially whatever still does
 * not join up.  The answers are exact whatever the guesses were.  The chunk minimum of such an image is 256 bytes (MFA_DFA_CHUNK sets
 * it); DESIGN.md section 4.9 has the sweep behind the three defaults.  Each chunk takes 144 bytes of the arena (about 25 MB
 * per overlapping launch).  The extra launches are there from the first call on (no quiet workspace: one long string walked whole costs
 * seconds).  MFA_SET_SPLIT=0 turns the path off for these images only, MFA_DFA_SPLIT=0 for all; MFA_DFA_SPLIT_MIN, MFA_DFA_CHUNK and
 * MFA_DFA_ARENA are shared with the tabulated engines.  mfa_last_set_split tells what the last call did; mfa_last_dfa_split and
 * mfa_last_dfa_spec answer zeros for such an image.  In a mixed object its segment always gets a launch of its own, which cuts long
 * strings in the same way.  mfa_last_kernel_ms covers the kernel and the launches behind it.  A string beyond MFA_MAX_STRING_BYTES
 * answers 2. */
int  mfa_image_create(const void* blob, size_t n_bytes, mfa_image_t** out);
void mfa_image_destroy(mfa_image_t* img);
int  mfa_image_get_info(const mfa_image_t* img, mfa_image_info* out);

/* Upload the image's tables to `device` and allocate its launch workspace now
 * (otherwise done by the first match call on that device). */
int  mfa_image_prepare(mfa_image_t* img, int device);

/* Every memory automaton is walked by the table-driven kernel (MFA_KERNEL_WALK) as soon as its image
 * exists: nothing is compiled per automaton.  A small automaton (up to 128 nodes) can ALSO be given a
 * kernel specialised to it (straight-line code, its state in registers: faster per input character on
 * text without periodic stretches): generated as HIP source, compiled for gfx950 with hipcc and cached
 * as a code object next to the library (or in $MFA_JIT_CACHE).  This call does that now; it is host-only
 * work and needs no GPU, so caches can be built ahead of time.  A match call uses the specialised kernel
 * when its code object is in the cache and never waits for a compiler (MFA_WALK=table / MFA_WALK=jit force
 * one kernel or the other; MFA_JIT=0 disables specialised kernels; MFA_ACCEL=0 or MFA_REGIONS=0: no region pass,
 * every step is executed -- A/B runs).  MFA_ERR_UNSUPPORTED: the automaton
 * is too large for a specialised kernel; MFA_ERR_JIT: the compiler failed. */
int  mfa_image_specialize(mfa_image_t* img);

/* Match n strings; string k is bytes[offsets[k] .. offsets[k+1]).  ALL pointers are
 * DEVICE pointers on `device` (offsets has n+1 entries; results gets n bytes, 1 =
 * accepted, 0 = rejected -- the value `cout << match` prints, match.cpp:30).
 * A string longer than MFA_MAX_STRING_BYTES is not matched: its result byte is set to 2.
 * The kernels read the batch in whole 16-byte blocks: d_bytes must be readable up to offsets[n]
 * rounded up to the next multiple of 16 (hipMalloc'ed buffers always are; a batch carved out of a
 * larger buffer needs up to 15 bytes of slack behind it).  The bytes there are never interpreted.
 * Asynchronous: work is enqueued on `stream` (a hipStream_t, NULL = default
 * stream) and the call returns.  Replaces: the loop
 *     while (...) { match = automata->match(text); }      match.cpp:21-31
 *
 * Long strings of a memory-less automaton (MFA_KIND_NFA).  The table kernels walk one string per lane, so a call would take as long
 * as its longest string.  A string of MFA_DFA_SPLIT_MIN bytes or more (default 65536) is therefore cut into chunks that are walked
 * side by side for every start state, and the chunks' state maps are composed in scan order: the time of a call follows the bytes
 * in the batch.  The answers are the same.  All of it runs inside this call on `stream`, with no read-back and no wait, so the call
 * stays asynchronous and legal inside a stream capture (once a first call has allocated the workspace).
 * Limits: memory-less automata only, every table size, both scan directions; memory automata are matched as before whatever the lengths.
 * "For every start state" holds for tables that live in LDS, up to 127 state sets.  A table kept in L2 (255 to MFA_MAX_DFA_STATES state
 * sets) has too many states for that: every chunk is walked from ONE state -- the first chunk from the true one, the others from a guess,
 * the state reached over the MFA_DFA_SPEC_LOOKBACK bytes (default 256) in front of the chunk from {start} or, if that walk dies, from a
 * "home" state chosen per image -- then MFA_DFA_SPEC_ROUNDS launches (default 3, at most 8; fixed when the call is enqueued) walk again every
 * chunk that was not started from what its predecessor ended in, and a last step follows each string's chunks from its true state and walks
 * serially whatever still does not join up.  The answers are exact whatever the guesses were; an automaton whose state never converges (a
 * counter such as (a^150)*) costs the time of the one-lane walk plus the rounds.  Both defaults are ESTIMATES until DESIGN.md section 4.8 has
 * the sweep.  Each chunk then takes 12 bytes of the arena (about 2.5 MB per overlapping launch).  MFA_DFA_SPEC=0 turns this off for the large
 * tables only.  mfa_last_dfa_spec tells what repairing cost.  For these tables a launch workspace starts in the quiet state described below:
 * the first batch with a long string that a workspace (one per stream in use) meets is walked whole, as every such batch was before, and from
 * its next call on long strings are cut, for good; MFA_DFA_SPLIT=2 cuts from the first call on.
 * At most 16384 long strings per call are cut, the others are walked
 * whole.  The chunk size is chosen on the device: max(MFA_DFA_CHUNK (default 4096), round_up(bytes of the long strings / 131072, 16)),
 * so the maps fit a fixed arena (about 1.1 to 22 MB per overlapping launch, by the number of state sets) whatever the batch holds.
 * A launch workspace (one per stream in use) whose last four calls met no long string leaves the extra launches out; the first batch
 * with long strings after that is walked whole, and from then on that workspace keeps the extra launches for good: the hint can cost one
 * slow batch per workspace, not one per batch, whatever the traffic looks like.  A stream capture records whichever form the call has at
 * capture time and every replay repeats it: capture after a call that had long strings, or with MFA_DFA_SPLIT=2, which always launches
 * the split kernels.  MFA_DFA_SPLIT=0 turns the path off (A/B runs).  A batch of 2^31 strings or more is not cut (the queue counts in 32 bits).
 * mfa_last_dfa_split tells what the last call did. */
int  mfa_match_batch(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                     uint8_t* d_results, int device, void* stream);

/* ---- strings in pieces (memory-less automata) -----------------------------------------------------
 * The walk of a tabulated automaton (MFA_KIND_NFA) is a fold over the input and its whole state between two bytes is ONE number, the
 * state set it is in.  The resume call takes that number in and hands it out, so a string may arrive in pieces -- a log in blocks, a
 * file larger than device memory, a string beyond MFA_MAX_STRING_BYTES -- one call per round of pieces.
 * Pointers, batch layout, the 16-byte read rule and asynchrony are those of the plain batch call above.  d_states: n words of device
 * memory, read and written in place: on entry word k is the state string k has reached so far (MFA_DFA_STATE_START for its first
 * piece), on return the state after this piece.  d_results may be NULL (a caller that wants the answer after the last piece only);
 * otherwise results[k] is what the plain call would answer for the concatenation of the pieces given so far.
 * The words are the image's plain state-set numbers.  They mean something only to images made from the same blob by the same build
 * of this library: DO NOT STORE THEM, and do not carry them from one automaton to another.
 * SCAN ORDER: pieces are given in the order the automaton scans.  For an image with is_reversed (mfa_image_info) that is from the
 * END of the string: its LAST piece goes into the first call, its first piece into the last.
 * Equivalence: cut a string into pieces anywhere, empty pieces included, and give them in scan order -- state and result byte are
 * those of one call on the whole string; a call on whole strings with every word MFA_DFA_STATE_START answers byte for byte what the
 * plain call answers.
 * Errors on the device are sticky: a word on entry that names no state set of the image (MFA_DFA_STATE_INVALID among them), or a
 * piece longer than MFA_MAX_STRING_BYTES, leaves MFA_DFA_STATE_INVALID and result 2, and so does every later call on that word.  The
 * SUM of a string's pieces has no limit.  A string that enters dead (MFA_DFA_STATE_DEAD) leaves dead with result 0 and its bytes are
 * not read.
 * Every table form is covered (LDS up to 127 state sets, L2 up to MFA_MAX_DFA_STATES; MFA_DFA_KERNEL=packed has no resume form and
 * takes the LDS table).  A piece of MFA_DFA_SPLIT_MIN bytes or more is cut across the GPU as described above, whatever the table's size --
 * on an LDS table the fold starts from the string's word, on an L2 table the piece's first chunk does -- with the same knobs, the same
 * quiet-workspace rule and the same report through the split-report calls below; a word that is dead or in error is never cut; the call is legal inside a stream capture under the same conditions and re-entrant per (image, device, stream).
 * MFA_ERR_UNSUPPORTED: a memory automaton (its state holds spans of the input; there is no number to hand over), or a set-walk image
 * (dfa_states == 0: its state is a set of nodes; the resume call for sets, further down, takes it).
 * MFA_ERR_INVALID_ARG: d_states is NULL.  Both are answered before the device is touched. */
#define MFA_DFA_STATE_DEAD    0u           /* the empty set: absorbing, rejecting */
#define MFA_DFA_STATE_START   1u           /* {start}: what a string's first piece is given */
#define MFA_DFA_STATE_INVALID 0xffffffffu
int  mfa_match_batch_resume(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                            uint32_t* d_states, uint8_t* d_results, int device, void* stream);
/* the same with HOST pointers (copy in, match, copy states and results out, synchronise); a piece beyond the limit is the sticky
 * error above, not MFA_ERR_TOO_LONG */
int  mfa_match_batch_resume_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                                 uint32_t* states, uint8_t* results, int device);

/* ---- strings in pieces (set-walk images) ------------------------------------------------------------
 * The state of a set-walk image (dfa_states == 0) between two bytes is the SET of live nodes.  This resume call takes that set in and hands it
 * out, in a record of 48 bytes per string, so a string may arrive in pieces exactly as with the call above -- one call per round of pieces.
 * Pointers, batch layout, the 16-byte read rule and asynchrony are those of the plain batch call.  d_states: n records of device
 * memory, 16-byte aligned, read and written in place: on entry record k says what string k has reached so far, on return what it has
 * reached behind this piece.  tag MFA_SET_STATE_START: the string's first piece, `nodes` is ignored -- a zero-filled buffer is "every
 * string at its start".  tag MFA_SET_STATE_LIVE: `nodes` is the set reached, node v being bit v & 31 of nodes[v >> 5]; the empty set is
 * dead, absorbing and rejecting.  On return the tag is MFA_SET_STATE_LIVE or MFA_SET_STATE_INVALID, `reserved` is zero and the words of
 * `nodes` beyond the image's mask width (1, 2, 4 or 8 words for up to 32, 64, 128, 256 nodes) are zero.  d_results may be NULL;
 * otherwise results[k] is what the plain call would answer for the concatenation of the pieces given so far: 0 for the empty set, else 1
 * if and only if the set holds a node from which `finish` is reached over epsilon edges alone.
 * The records hold the image's own node numbers.  They mean something only to images made from the same blob by the same build
 * of this library: DO NOT STORE THEM, and do not carry them from one automaton to another.
 * SCAN ORDER: pieces are given in the order the automaton scans.  For an image with is_reversed that is from the END of the string:
 * its LAST piece goes into the first call, its first piece into the last.
 * Equivalence: cut a string into pieces anywhere, empty pieces included, and give them in scan order -- the final record and the final
 * result byte are those of one call on the whole string from a zeroed record; such a call on whole strings answers byte for byte what
 * the plain call answers.
 * Errors on the device are sticky: a tag other than START or LIVE (INVALID among them), a `reserved` word that is not zero, a bit set for
 * a node the image does not have (any word beyond its mask width included), a piece longer than MFA_MAX_STRING_BYTES, or a walk whose
 * stack would overflow (the record names nodes no walk of this image reaches together) leaves tag MFA_SET_STATE_INVALID, `nodes` zero and
 * result 2, and so does every later call on that record.  The SUM of a string's pieces has no limit.  A record that enters LIVE with the
 * empty set leaves the same with result 0 and its bytes are not read.
 * A piece of MFA_DFA_SPLIT_MIN bytes or more that enters with a live set is cut across the device as mfa_match_batch cuts a long string
 * (mfa_image_create has the scheme and the knobs): its first chunk starts from the record's set, and the record and the result byte are
 * written by the last launch.  Dead, invalid and over-long records are answered as before.  mfa_last_set_split tells what the call did
 * (mfa_last_dfa_split and mfa_last_dfa_spec answer zeros); last_kernel becomes
 * MFA_KERNEL_NODESET and mfa_last_kernel_ms covers the launches.  Re-entrant per (image, device, stream), and legal inside a stream capture
 * once a first call has run (it allocates the workspace and raises the kernel's LDS limit).
 * MFA_ERR_INVALID_ARG: img, d_offsets or d_states is NULL, or d_states is not 16-byte aligned.  MFA_ERR_UNSUPPORTED: a memory automaton,
 * a tabulated image (dfa_states != 0: its state is one number and the call above carries it), or a wave image (more than 256 nodes, or
 * made under MFA_SET_WAVE=1: its set may take 64 words and a record has eight; the records are left as they came).  All are answered
 * before the device is touched; n == 0 is MFA_OK. */
#define MFA_SET_STATE_START   0u           /* first piece; `nodes` is ignored.  A zero-filled buffer is "every string at its start" */
#define MFA_SET_STATE_LIVE    1u           /* `nodes` is the set reached so far; the empty set is dead: absorbing, rejecting */
#define MFA_SET_STATE_INVALID 0xffffffffu  /* sticky error */
typedef struct mfa_set_state { uint32_t tag; uint32_t reserved[3]; uint32_t nodes[8]; } mfa_set_state;   /* 48 bytes */
int  mfa_match_batch_resume_set(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                                mfa_set_state* d_states, uint8_t* d_results, int device, void* stream);
/* the same with HOST pointers (copy in, match, copy records and results out, synchronise; `states` needs no alignment beyond its type's);
 * a piece beyond the limit is the sticky error above, not MFA_ERR_TOO_LONG */
int  mfa_match_batch_resume_set_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                                     mfa_set_state* states, uint8_t* results, int device);

/* ---- strings in pieces (wave images) ----------------------------------------------------------------
 * A wave image (a set-walk image of more than 256 nodes, or one made under MFA_SET_WAVE=1) holds its set across the 64 lanes of a wave:
 * up to 64 words.  Its record is mfa_set_state_wide, 272 bytes per string -- the tag quarter of mfa_set_state and nodes[64] -- and its
 * call is mfa_match_batch_resume_set_wide.  The contract is that of mfa_match_batch_resume_set above with nodes[64] in place of
 * nodes[8]: pointers, batch layout, the 16-byte read rule, asynchrony and scan order; d_states is n records of device memory, 16-byte
 * aligned, read and written in place; the tags are MFA_SET_STATE_START (`nodes` is ignored: a zero-filled buffer is "every string at
 * its start"), MFA_SET_STATE_LIVE (node v is bit v & 31 of nodes[v >> 5]; the empty set is dead) and MFA_SET_STATE_INVALID.  On return
 * the tag is LIVE or INVALID, `reserved` is zero and every word of `nodes` at and beyond the image's W = ceil(n_nodes / 32) is zero.
 * d_results may be NULL; otherwise results[k] is what the plain call would answer for the concatenation of the pieces given so far.
 * Equivalence, "do not store them" and the sticky errors are as above: a tag other than START or LIVE, a `reserved` word that is not
 * zero, a bit for a node the image lacks (any word at or beyond W included), a piece longer than MFA_MAX_STRING_BYTES or a stack
 * overflow leaves tag MFA_SET_STATE_INVALID, `nodes` zero and result 2, and so does every later call on that record.  The SUM of a
 * string's pieces has no limit.  A record that enters LIVE with the empty set leaves as it came with result 0 and its bytes are not read.
 * Long pieces: a piece of MFA_DFA_SPLIT_MIN bytes or more (and within MFA_MAX_STRING_BYTES) whose record holds a live set that is not
 * empty is cut into chunks inside the same call, a wave per chunk, as mfa_match_batch cuts a long string of such an image
 * (mfa_image_create above); the first chunk starts from the record's set, and the record gets the set reached.  Dead, invalid and
 * over-long records are answered as before, by the main kernel (nfa_set_wave_resume_kernel).  mfa_last_set_split tells what the call
 * did (zeros when no piece was queued).  last_kernel becomes MFA_KERNEL_NODESET and mfa_last_kernel_ms covers the kernel and the
 * launches behind it.  Re-entrant per (image, device, stream), and legal inside a stream capture once a first call has run (it
 * allocates the workspace and raises the kernels' LDS limit).
 * MFA_ERR_INVALID_ARG: img, d_offsets or d_states is NULL, or d_states is not 16-byte aligned.  MFA_ERR_UNSUPPORTED, with the records
 * as they came: a memory automaton, a tabulated image, or a lane image (a set-walk image of up to 256 nodes made without
 * MFA_SET_WAVE=1: its call is the 48-byte one).  All are answered before the device is touched; n == 0 is MFA_OK. */
typedef struct mfa_set_state_wide { uint32_t tag; uint32_t reserved[3]; uint32_t nodes[64]; } mfa_set_state_wide;   /* 272 bytes: 17 quarters of 16 */
int  mfa_match_batch_resume_set_wide(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                                     mfa_set_state_wide* d_states, uint8_t* d_results, int device, void* stream);
/* the same with HOST pointers (copy in, match, copy records and results out, synchronise; `states` needs no alignment beyond its type's);
 * a piece beyond the limit is the sticky error above, not MFA_ERR_TOO_LONG */
int  mfa_match_batch_resume_set_wide_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                                          mfa_set_state_wide* states, uint8_t* results, int device);

/* Which resume call an image takes, as the bytes of one string's state: 0 for a memory automaton (nothing is carried), 4 for a
 * tabulated image (mfa_match_batch_resume), 48 for a lane set-walk image (mfa_match_batch_resume_set), 272 for a wave image
 * (mfa_match_batch_resume_set_wide).  Touches no device.  MFA_ERR_INVALID_ARG: img or bytes is NULL. */
int  mfa_image_resume_state_bytes(mfa_image_t* img, uint32_t* bytes);

/* ---- region tables -------------------------------------------------------------------------------
 * Before a memory automaton walks a batch, one streaming pass over the batch (region_scan_kernel)
 * finds every string's periodic regions -- stretches with s[j] == s[j+q], q <= 8 -- and leaves them in
 * a table the walk kernels look up instead of measuring the stretches themselves.  mfa_match_batch
 * runs that pass itself; it is exported for callers that match SEVERAL automata against the same
 * batch (mfa_match_batch_regions: the pass then runs once) and for tests.
 * Table layout: MFA_REGION_WORDS uint64 per string; word 0 = count | flags, then `count` entries
 *   lo | hi << 24 | q << 48     (offsets relative to the start of the string, memory order)
 * Every entry is true (s[j] == s[j+q] for lo <= j < hi - q) and entries with q = 1 are maximal runs.
 * MFA_REGION_OVERFLOW in word 0: the string has more regions than fit and the table holds the first three and the longest of the others
 * (or the string is too long to be matched): the walk then executes the other stretches step by step. */
#define MFA_REGION_WORDS    16u
#define MFA_REGION_MAX      15u
#define MFA_REGION_OVERFLOW 0x100ull
#define MFA_REGION_MIN_LEN  64u

/* d_table: device buffer of n * MFA_REGION_WORDS uint64.  Asynchronous on `stream`. */
int  mfa_region_scan(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t* d_table,
                     int device, void* stream);

/* mfa_match_batch with a region table the caller has already filled for this batch on this stream
 * (or on a stream this one waits for).  d_table == NULL: no table, every step is executed. */
int  mfa_match_batch_regions(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                             uint8_t* d_results, const uint64_t* d_table, int device, void* stream);

/* ---- mixed batches --------------------------------------------------------------------------------
 * ONE batch whose strings belong to several automata, segment by segment (the 10-example attack
 * corpus is one byte buffer, one offset array and ten segments).  Replaces: running the loop of
 * match.cpp:21-31 once per automaton.  A mixed object holds the automata's tables back to back, per
 * device; the images must outlive it, and its memory automata scan in the same direction and fit the table-driven walk
 * (MFA_ERR_UNSUPPORTED otherwise).  One call runs the region pass over the batch in a few groups of
 * consecutive segments and walks each group -- all its automata in ONE launch, any lane any automaton --
 * as soon as its regions are known: the region launches go to `stream` itself, the walks to internal streams, so that
 * the walk of a group runs beside the region pass of the next (one region launch per group, the walks wait for the event
 * behind it).  Calls on one object are ordered one behind the other, also when they come on different streams (the object's
 * table and work areas are shared).  `stream` sees the call as a single operation: it waits for the internal streams before the call
 * returns, ALSO when the call returns an error (whatever was started is ordered before the caller's next
 * operation on `stream`).
 *
 * Memory-less automata (MFA_KIND_NFA) in a mixed object.  The images may be of either kind, in any order; a memory-less one may scan in
 * either direction whatever the others do.  Memory-less segments have no use for regions: the region launches are clipped to the runs of
 * memory segments (an object without a memory automaton launches none, and mfa_mixed_last_ms reports region_ms 0), and the memory-less
 * segments are walked on an internal stream of their own, behind the call's entry only, beside the region launches.  With MFA_MIXED_DFA=1
 * every segment whose table fits the tiled table kernel -- table plus input tile at most 64 KiB of LDS, up to 55 state sets -- shares ONE launch of
 * dfa_mixed_kernel: any workgroup any automaton, a workgroup reloads its table only when the automaton changes.  Every other memory-less
 * segment gets a launch of its own, exactly mfa_match_batch on its strings: larger tables, every memory-less segment when MFA_WALK=jit
 * selects the per-segment schedule, and segments of MFA_MIXED_DFA_OWN strings or more (default 32768), for which a launch of their own is
 * the better deal.  MFA_MIXED_DFA=0, the DEFAULT until the shared launch has been measured against the per-image calls (the 32768 is
 * an estimate for the same reason), gives every memory-less segment its own launch.  Both are read per call.
 * Inside the shared launch a string of MFA_DFA_SPLIT_MIN bytes or more is walked WHOLE by its lane -- the call then takes as long as that
 * string; only launches of their own have the split path for long strings.  Such a corpus belongs in mfa_match_batch, or its segment in a
 * launch of its own (MFA_MIXED_DFA_OWN).  Result bytes: 0 or 1; the shared launch answers a string beyond MFA_MAX_STRING_BYTES with 2 and
 * does not walk it, a launch of its own answers what mfa_match_batch answers for that image.
 * Nothing is read back and nothing is uploaded per call (the segments travel as kernel arguments), so a call stays legal inside a
 * stream capture under the conditions above, once a first call has uploaded the tables.  mfa_mixed_last_dfa tells what the last call did. */
typedef struct mfa_mixed mfa_mixed_t;
int  mfa_mixed_create(mfa_image_t* const* images, uint32_t n_images, mfa_mixed_t** out);
void mfa_mixed_destroy(mfa_mixed_t* mx);
/* seg_first: HOST array of n_images + 1 string indices, seg_first[0] = 0, seg_first[n_images] = n: strings
 * seg_first[s] .. seg_first[s+1]-1 are matched against images[s].  Device pointers as in mfa_match_batch.
 * Asynchronous on `stream` -- except that the first call with a string count this object has not met (n >= 65536) reads the
 * batch's size in bytes back (offsets[n] - offsets[0]) to choose the number of groups, and waits for `stream` to do so
 * (make such a call outside a stream capture, or use mfa_match_mixed_sized), and that with the generated kernels (MFA_WALK=jit)
 * the first call on a device times the walks and synchronises on its own end.  A later batch with the same string count and
 * other bytes is grouped like the first: a matter of speed only. */
int  mfa_match_mixed(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                     const uint64_t* seg_first, uint8_t* d_results, int device, void* stream);
/* the same for a caller that knows the batch's size in bytes (total_bytes = offsets[n] - offsets[0], > 0): nothing is read back,
 * the call never waits for `stream` */
int  mfa_match_mixed_sized(mfa_mixed_t* mx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint64_t total_bytes,
                           const uint64_t* seg_first, uint8_t* d_results, int device, void* stream);
/* the same with HOST pointers (copy in, match, copy out, synchronise): for callers that hold std::strings */
int  mfa_match_mixed_host(mfa_mixed_t* mx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                          const uint64_t* seg_first, uint8_t* results, int device);
/* device time of the last mfa_match_mixed call on `device`: its region launches, and first region launch to
 * last walk (either pointer may be NULL).  Synchronises on the call's last events. */
int  mfa_mixed_last_ms(mfa_mixed_t* mx, int device, float* region_ms, float* span_ms);
/* the same for the call `back` calls ago (0 = the last one; the events of the last 32 calls are kept, so a sequence of calls can be
 * timed without synchronising between them) */
int  mfa_mixed_timing(mfa_mixed_t* mx, int device, uint32_t back, float* region_ms, float* span_ms);
/* what the last call on `device` launched (any pointer may be NULL): region launches, walk launches, groups of strings, and
 * gated, always 0 (kept for compatibility) */
int  mfa_mixed_last_launches(mfa_mixed_t* mx, int device, uint32_t* region_launches, uint32_t* walk_launches, uint32_t* groups, uint32_t* gated);
/* what the last call on `device` did with its memory-less segments (any pointer may be NULL): launches of the multi-table kernel, launches of
 * single segments, and the items (segments) and strings inside the multi-table launches.  The walk launches of mfa_mixed_last_launches are
 * memory-automaton walks only.  Same locking and errors as mfa_mixed_last_launches. */
int  mfa_mixed_last_dfa(mfa_mixed_t* mx, int device, uint32_t* multi_launches, uint32_t* own_launches, uint32_t* items, uint64_t* strings);

/* The result vector of a batch as a bitmap: bit k % 8 of byte k / 8 of d_bitmap ((n + 7) / 8 bytes, device memory) = string k was accepted
 * (result code 1).  Asynchronous on `stream`.  What a process sends when the results of a batch sharded over several GPUs are gathered
 * (the reference matches one string at a time and has no such step: matchers/match_mfa.cpp:28-36 prints each answer as it comes). */
int  mfa_pack_result_bitmap(const uint8_t* d_results, uint64_t n, uint8_t* d_bitmap, void* stream);

/* ---- text to batch ---------------------------------------------------------------------------------
 * Every match entry point takes a batch: strings back to back in `bytes`, bounded by offsets[0..n], no separators between them.  These
 * calls make that batch from a TEXT in device memory -- a file, a log, the rest of stdin -- on the device: separators found, strings
 * counted, kept bytes compacted, offsets written.  Replaces: the extraction half of the per-string loops, `cin >> text`
 * (matchers/match.cpp:21-31) and std::getline (matchers/match_mfa.cpp:28-36,72-80).
 * The rule.  MFA_SPLIT_LINES restates std::getline(file, line): a string ends at byte 0x0a, which is dropped; every other byte is kept,
 * \r and NUL included; empty lines are strings (two equal offsets); bytes behind the last 0x0a form a last string only if there is at
 * least one of them ("" gives 0 strings, "\n" one empty string, "a\nb" and "a\nb\n" both 2).  MFA_SPLIT_TOKENS restates `cin >> text`
 * in the C locale: separators are 0x09..0x0d and 0x20, a string is a maximal run of other bytes, there are no empty strings.  An
 * optional stop token (tokens mode only; 1 to 15 bytes, none of them a separator; the command line passes "exit") ends the batch at the
 * first token EQUAL to it: the strings are the tokens in front of it.  A token that merely starts or ends with it does not stop; a stop
 * token at the very end of the text, with no separator behind it, does.
 * Two calls.  mfa_split_text_count counts: it fills the workspace (mfa_split_workspace_bytes(n_text_bytes) bytes of device memory,
 * 16-byte aligned) and the n_strings, n_bytes and stopped fields of *d_info (device memory, 8-byte aligned), and zeroes the other two.
 * mfa_split_text_write writes the batch into d_bytes (bytes_capacity bytes) and d_offsets (max_strings + 1 entries) and sets
 * max_string_bytes and overflow.  The text is cut into tiles of mfa_split_tile_bytes(); the passes are plain launches in stream
 * order, no workgroup waits for another.
 * Asynchrony and order.  Both calls are asynchronous on `stream`.  `write` uses the workspace and the info record that a `count` of the
 * same text, mode and stop token left; the two calls may follow each other on one stream with no wait in between when the caller can
 * bound the sizes itself (a text of t bytes holds at most t kept bytes, t + 1 lines, (t + 1) / 2 tokens); otherwise the caller reads
 * the 32 bytes of the info back between them and allocates exactly.
 * Input.  d_text is 16-byte aligned and readable up to n_text_bytes rounded up to 16; the bytes there are never interpreted.
 * Output capacity.  A d_bytes of capacity round_up(n_bytes, 16) satisfies the read rule of mfa_match_batch.  d_bytes needs no alignment.
 * What is valid after `write`: offsets[0] = 0; offsets[0 .. min(n_strings, max_strings)] are valid, and so is d_bytes[0 .. offsets[that])
 * as far as bytes_capacity reaches.  Everything else in the two buffers inside their capacities is unspecified; everything outside them
 * is untouched: no offset with an index above max_strings is written, and no byte at or beyond bytes_capacity.
 * Overflow.  `overflow` is set when anything was clipped, by max_strings or by bytes_capacity.  The counts in the info are still the
 * true ones, so the caller can allocate and call `write` again.
 * n_text_bytes == 0 (d_text may then be NULL): MFA_OK, 0 strings, offsets[0] = 0, no tile launched.
 * MFA_ERR_INVALID_ARG, answered before the device is touched: a NULL pointer (d_bytes may be NULL when bytes_capacity is 0); an unknown
 * mode; a stop token in lines mode; a stop token that is empty, longer than 15 bytes or holds a separator; a d_text or d_workspace that
 * is not 16-byte aligned, a d_info or d_offsets that is not 8-byte aligned; a text of 2^45 bytes or more.  MFA_ERR_NO_DEVICE as
 * everywhere else.
 * Long strings.  The splitter does not look at MFA_MAX_STRING_BYTES: a longer string is answered 2 by the match call, as always;
 * max_string_bytes lets a caller see it coming. */
#define MFA_SPLIT_LINES  0u
#define MFA_SPLIT_TOKENS 1u
typedef struct mfa_split_info {      /* device memory, 32 bytes */
    uint64_t n_strings;              /* true count (in front of the stop token, if one was met), whatever max_strings is */
    uint64_t n_bytes;                /* kept bytes of those strings = offsets[n_strings] */
    uint64_t max_string_bytes;       /* written by mfa_split_text_write: over the strings it wrote */
    uint32_t stopped, overflow;      /* stop token met; write clipped by max_strings or bytes_capacity */
} mfa_split_info;
uint32_t mfa_split_tile_bytes(void);
/* MFA_ERR_INVALID_ARG: bytes is NULL, or the text is too long (above) */
int mfa_split_workspace_bytes(uint64_t n_text_bytes, size_t* bytes);
int mfa_split_text_count(const uint8_t* d_text, uint64_t n_text_bytes, uint32_t mode, const char* stop_token,
                         void* d_workspace, mfa_split_info* d_info, int device, void* stream);
int mfa_split_text_write(const uint8_t* d_text, uint64_t n_text_bytes, uint32_t mode,
                         const void* d_workspace, mfa_split_info* d_info,
                         uint8_t* d_bytes, uint64_t bytes_capacity, uint64_t* d_offsets, uint64_t max_strings,
                         int device, void* stream);

/* ---- batch to text ---------------------------------------------------------------------------------
 * The way out of a batch: the strings that a match call answered 1 -- or 0, with MFA_SELECT_INVERT -- compacted on the device, so that
 * only what matched travels back: their bytes back to back as a batch of their own, or with a 0x0a behind each as a text
 * (MFA_SELECT_NEWLINE), their offsets in the output and their indices in the input.  What `grep -x` and `grep -vx` print.  Replaces: the
 * join of the answers with the input that the per-string loops leave to their caller (matchers/match_mfa.cpp:28-36 prints one answer
 * per line).
 * Input.  A batch exactly as mfa_match_batch takes it: offsets[0] need not be 0, d_bytes needs no alignment.  d_results is what a match
 * call left for it, one byte per string.  String k is kept when d_results[k] is 1, or 0 under MFA_SELECT_INVERT.  Every other value (2:
 * beyond MFA_MAX_STRING_BYTES) is never kept, with either flag, and is counted in n_unanswered.
 * Read rule.  The calls read no byte outside the aligned 16-byte blocks of memory that [d_bytes + offsets[0], d_bytes + offsets[n])
 * touches: narrower than what mfa_match_batch asks for.  They read d_results[0 .. n) and d_offsets[0 .. n].
 * Two calls.  mfa_select_count fills the workspace (mfa_select_workspace_bytes(n) bytes of device memory, 16-byte aligned) and the counts
 * of *d_info (device memory, 8-byte aligned), and zeroes overflow.  mfa_select_write writes the kept strings and sets overflow.  The
 * passes are plain launches in stream order, no workgroup waits for another; the bytes are moved by one workgroup per 16 KiB of OUTPUT,
 * so a batch of one long string beside a million empty ones is spread like any other.
 * Output.  Kept strings appear in batch order.  d_out_indices[r] is the index k of the r-th kept string (d_out_indices may be NULL),
 * d_out_offsets[r] where its bytes start in d_out_bytes; d_out_offsets[0] = 0 and d_out_offsets[n_selected] = n_bytes.  Without
 * MFA_SELECT_NEWLINE the two output buffers are themselves a batch for any match call (empty strings leave equal offsets), and a
 * bytes_capacity of round_up(n_bytes, 16) satisfies the read rule of mfa_match_batch.  With it, string r occupies
 * [out_offsets[r], out_offsets[r+1] - 1) and the byte behind it is 0x0a: d_out_bytes[0 .. n_bytes) is a text that mfa_split_text_* in
 * lines mode cuts back into the same strings, provided no kept string holds a 0x0a.  d_out_bytes needs no alignment; it may be NULL when
 * bytes_capacity is 0, which gives indices and offsets only (overflow is then set unless n_bytes is 0).
 * Validity and clipping, as for mfa_split_text_write.  With v = min(n_selected, max_selected), valid after `write` are
 * out_offsets[0 .. v], out_indices[0 .. v) and out_bytes[0 .. min(out_offsets[v], bytes_capacity)).  Everything else inside the
 * capacities is unspecified; everything outside them is untouched: nothing above out_offsets[max_selected] or
 * out_indices[max_selected - 1] is ever written, and no byte at or beyond bytes_capacity.  `overflow` is set when anything was clipped, by
 * max_selected or by bytes_capacity; the counts stay the true ones, so the caller can allocate and call `write` again.  The outputs must
 * not overlap the inputs or each other.
 * Asynchrony and order.  Both calls are asynchronous on `stream`.  `write` uses the workspace and the info record that a `count` of the
 * same results, offsets, n and flags left.  The two may follow each other on one stream with no wait in between when the caller bounds
 * the sizes itself: at most n strings, at most offsets[n] - offsets[0] bytes (+ n with MFA_SELECT_NEWLINE); otherwise the caller reads
 * the 32 bytes of the info back between them and allocates exactly.  Both calls are legal inside a stream capture: they make no
 * allocation, no read-back and no upload.
 * n == 0: MFA_OK, all counts 0, out_offsets[0] = 0.
 * MFA_ERR_INVALID_ARG, answered before the device is touched: a NULL pointer other than the two allowed above; unknown flag bits; a
 * d_workspace that is not 16-byte aligned; a d_info, d_offsets, d_out_offsets or d_out_indices that is not 8-byte aligned; an n of 2^40 or
 * more.  MFA_ERR_NO_DEVICE as everywhere else. */
#define MFA_SELECT_INVERT  1u  /* keep the strings answered 0 instead of those answered 1 */
#define MFA_SELECT_NEWLINE 2u  /* one byte 0x0a behind every kept string: the output is a text */
typedef struct mfa_select_info {     /* device memory, 32 bytes, 8-byte aligned */
    uint64_t n_selected;             /* true count, whatever max_selected is */
    uint64_t n_bytes;                /* output bytes of those strings: their lengths, plus n_selected with NEWLINE */
    uint64_t n_unanswered;           /* strings whose result byte is neither 0 nor 1 (2: beyond MFA_MAX_STRING_BYTES); never kept */
    uint32_t overflow, reserved;     /* write clipped by max_selected or bytes_capacity; zero */
} mfa_select_info;
/* MFA_ERR_INVALID_ARG: bytes is NULL, or n_strings is 2^40 or more */
int mfa_select_workspace_bytes(uint64_t n_strings, size_t* bytes);
int mfa_select_count(const uint8_t* d_results, const uint64_t* d_offsets, uint64_t n, uint32_t flags,
                     void* d_workspace, mfa_select_info* d_info, int device, void* stream);
int mfa_select_write(const uint8_t* d_bytes, const uint64_t* d_offsets, const uint8_t* d_results, uint64_t n, uint32_t flags,
                     const void* d_workspace, mfa_select_info* d_info,
                     uint8_t* d_out_bytes, uint64_t bytes_capacity, uint64_t* d_out_offsets, uint64_t* d_out_indices,
                     uint64_t max_selected, int device, void* stream);

/* ---- search inside lines ---------------------------------------------------------------------------
 * Where every match call answers "is the whole string in the language", this one finds the leftmost-longest match INSIDE every string
 * of a batch: what `grep` (results) and `grep -o` (spans) ask.  For a tabulated memory-less image (kind NFA, 2 to 127 state sets).
 * Definition.  For string k = bytes[b .. e), a match is a pair b <= i <= j <= e such that mfa_match_batch on this image would answer 1
 * for bytes[i .. j) taken as a string of its own (an is_reversed image scans that substring from its end, as always).  Reported is the
 * smallest such i and, for it, the largest j.  Empty matches count: an automaton that accepts the empty string finds i = b everywhere.
 * Outputs.  Found: d_results[k] = 1, d_spans[2k] = i, d_spans[2k+1] = j -- absolute positions in d_bytes, like the offsets.  Not found:
 * d_results[k] = 0 and d_spans[2k] = d_spans[2k+1] = b.  A string beyond MFA_MAX_STRING_BYTES is not read: d_results[k] = 2 and an empty
 * span at b.  d_spans[2n] = d_offsets[n].  d_spans[0 .. 2n] never decreases, so it is itself the offsets array of 2n strings over the
 * same d_bytes: string 2k is line k's match, string 2k+1 the text between it and the next line's match.  d_span_results (2n bytes) gets
 * [2k] = d_results[k] and [2k+1] = 0: with it mfa_select_count / mfa_select_write on (d_bytes, d_spans, d_span_results, 2n) and
 * MFA_SELECT_NEWLINE print every line's match on the device; their indices / 2 are the line numbers.
 * d_spans may be NULL (results only: the second pass is not launched); d_span_results may be NULL, and needs d_spans.
 * How.  Two walks per line over two tables derived from the image's own table (csrc/search_tables.h), built by the first call or by
 * mfa_image_search_info under the image's lock: one from the line's end down, which reads every byte of the batch once and finds i,
 * and one from i up until no match can go on, which finds j.  One lane walks one line in each pass.
 * The read rule is mfa_match_batch's: whole aligned 16-byte blocks up to d_offsets[n] rounded up to 16.
 * Asynchronous on `stream`; re-entrant per (image, device, stream); legal inside a stream capture once a first call on the device has
 * uploaded the tables.  last_kernel becomes MFA_KERNEL_SEARCH and mfa_last_kernel_ms covers both passes.
 * n == 0: MFA_OK, and d_spans[0] = d_offsets[0] when d_spans is given.
 * MFA_ERR_INVALID_ARG: img, d_offsets or d_results NULL; d_span_results without d_spans; a d_spans that is not 8-byte aligned.
 * MFA_ERR_UNSUPPORTED, answered before the device is touched, every output untouched: a memory automaton, a set-walk image, an image
 * of more than 127 state sets, an image one of whose two tables passes 127 sets (mfa_image_search_info answers the same).
 * mfa_search_batch_host: host pointers, as mfa_match_batch_host (spans and span_results may be NULL; a string beyond the limit is
 * MFA_ERR_TOO_LONG).  mfa_image_search_info: the sets of the two tables, the dead set included (0: the image accepts nothing). */
int mfa_search_batch(mfa_image_t* img, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                     uint8_t* d_results, uint64_t* d_spans, uint8_t* d_span_results, int device, void* stream);
int mfa_search_batch_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                          uint8_t* results, uint64_t* spans, uint8_t* span_results, int device);
int mfa_image_search_info(mfa_image_t* img, uint32_t* pass1_states, uint32_t* pass2_states);

/* Same with HOST pointers: copies the batch to the device, matches, copies the
 * results back, synchronises.  Convenience for callers that hold std::strings
 * (the CLI); throughput is then bounded by the host link, not by the kernel. */
int  mfa_match_batch_host(mfa_image_t* img, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                          uint8_t* results, int device);

/* Device-side time of the last match kernel launched through this image on
 * `device`, in milliseconds, measured with HIP events recorded on the launch stream
 * around the kernel alone (for a memory-less image: the table kernel and the kernels of the split path behind it -- plan, chunk and
 * fold, or for a table in L2 plan, chunk walk, repair rounds and resolve; a resume call is covered in the same way).  Synchronises on the stop event. */
int  mfa_last_kernel_ms(mfa_image_t* img, int device, float* ms);
/* What the split path of the last match call on this image and device did (any pointer may be NULL):
 * strings it took, chunks it cut them into, the chunk size in bytes the device chose.
 * All 0 when the path did not run (no long string, a memory automaton, MFA_DFA_SPLIT=0, a table in L2 with MFA_DFA_SPEC=0, or a call
 * that left the split launches out because its workspace had met no long string lately).
 * Synchronises on that call's last event and reads the figures back with a blocking copy, holding the image's lock: for tests and tools. */
int  mfa_last_dfa_split(mfa_image_t* img, int device, uint64_t* strings, uint64_t* chunks, uint32_t* chunk_bytes);
/* What repairing the guesses cost in the last match call on this image and device, for a table in L2 (any pointer may be NULL): chunks
 * walked again by the repair rounds, strings whose chunks still did not join up so that the last step walked their rest serially, and the
 * bytes walked that way.  All 0 when that path did not run (see above; an LDS table has no guesses).  Same locking, synchronisation and
 * errors as mfa_last_dfa_split. */
int  mfa_last_dfa_spec(mfa_image_t* img, int device, uint64_t* rewalked_chunks, uint64_t* serial_strings, uint64_t* serial_bytes);
/* What cutting long strings did in the last match call on this SET-WALK image and device (mfa_match_batch, mfa_match_batch_resume_set; any
 * pointer may be NULL): strings taken, chunks they were cut into, the chunk size in bytes the device chose, chunks walked again by the
 * repair rounds, strings whose chunks still did not join up so that the last step walked their rest serially, and the bytes walked that
 * way.  All 0 when the path did not run (no long string, another kind of image, MFA_SET_SPLIT=0, MFA_DFA_SPLIT=0).  Same locking,
 * synchronisation and errors as mfa_last_dfa_split. */
int  mfa_last_set_split(mfa_image_t* img, int device, uint64_t* strings, uint64_t* chunks, uint32_t* chunk_bytes, uint64_t* rewalked_chunks,
                        uint64_t* serial_strings, uint64_t* serial_bytes);
/* Device-side time of the region pass of that launch (0 if it ran none). */
int  mfa_last_region_ms(mfa_image_t* img, int device, float* ms);

int         mfa_device_count(void);        /* >= 0, or MFA_ERR_NO_DEVICE */
int         mfa_last_hip_error(void);      /* hipError_t of the last failed HIP call on this thread */
const char* mfa_strerror(int code);
const char* mfa_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MFA_HIP_H */
