// lz4_window_engine.inc — the lean exact-window parse of lz4_compress.hip as ONE hand-written gfx950 block.
//
// Included inside lz4_compress_wave<>() (kWindows path).  It runs whole 64-byte windows — table read, candidate
// gather, duplicate-hash passes, per-lane event records, the run loop, commit, ip-2 put, advance — for as long as
// the window conditions hold and only COMMON events occur, and hands back to the C++ code
//   code 0  at a window boundary whose conditions fail (the general batch or the C++ window path goes on),
//   code 2  in the middle of a window at the first event the block does not handle (the C++ run loop resumes at
//           exactly that event with the window's state: h, cp, info, Dp, ED, K, rs, valid, pend_q),
//   (code 3, "last literals", is no longer produced here: the block does not run within 384 bytes of the chunk's end)
//   (code 4 is no longer produced: a no-match run that leaves the consecutive-probe part of its schedule comes out
//   with t0 = 66 > 48 and code 0, and the C++ dispatch sends it to the general batch).
// Same arithmetic as the C++ window path (tests/model/lz4_window_model.cpp is the lock-step model of both); what
// it removes is the ~260 instructions and ~13 taken branches per window hipcc spends around the run loop
// (structurised control flow of the multi-exit loops, mask materialisation, register shuffling), see DESIGN.md §6.1.
// tests/isa runs this text on the CPU (gfx950 interpreter) against the oracle; tests/isa/hazards.py checks the
// wait states the hardware needs and hipcc does not insert inside an asm statement.
//
// Registers: operands are the C++ variables; fixed scratch (clobbered): s72-s99, v120-v167, and for the deferred emission m0 (the
// number of waiting sequences), v118 / v119 (their records, one lane each) and v97-v117 (the flush's scratch) - registers the
// compiled code around the block does not reach (it ends at v96; the kernel stays at 168 VGPRs = three wavefronts per SIMD).
//   s76 wbase   s77 0x80000 (the "forward length capped" bit of an event record)   s78 rs0   s79 hash multiplier
//   s[74:75] live lanes of the window (preparation)
//   s[80:81] lanes of the current run   s86 event lane   s87 its record   s88 candidate   s89 ip0   s90 fwd
//   s91 nb   s92 ip0-anchor   s93 lit   s94 mcode   s95 sequence bytes   s96 len - 384 (whole block)
//   v129 lane   v148 p   v149 LDS address of T[h]   v[144:147] gathered candidate bytes
//   v[132:135] v[136:139] v[140:143]  the 16 stream bytes p-4..p+11 of every lane for this window and the next two;
//   the three register sets rotate roles (three copies of the window body), so nothing is moved between windows.

#if defined(S3S_ENGINE_NO_SPEC)
#undef S3S_ENGINE_SPEC
#elif !defined(S3S_ENGINE_SPEC)
#define S3S_ENGINE_SPEC 1  /* shipped since round 5; -DS3S_ENGINE_NO_SPEC builds the round-4 block (A/B, tests) */
#endif

// Deferred emission (round 5, second half): a sequence's bytes are not built and stored in the run loop; the loop leaves a
// two-dword record (offset | anchor << 16, literal length | match code << 4) in lane m0 of v118 / v119 and .Lw_flush writes
// up to 64 sequences at once, one per lane (see S3S_ENGINE_FLUSH).  -DS3S_ENGINE_NO_DEFER builds the immediate form (A/B).
#if defined(S3S_ENGINE_NO_DEFER) || !defined(S3S_ENGINE_SPEC)
#undef S3S_ENGINE_DEFER
#elif !defined(S3S_ENGINE_DEFER)
#define S3S_ENGINE_DEFER 1
#endif

// THE NEXT WINDOW'S DUPLICATE PASSES RUN DURING THIS WINDOW (round 7).  Dp of window W + 64 depends only on its lanes' hashes,
// and those (v155 / v156) exist at W's head.  The head used to run W's own two passes - two dependent LDS round trips, the
// second with only the run-loop state in its shadow - before the run loop could start, because ED needs Dp.  Now W's head
// issues pass 1 of W + 64 next to the speculative table read it waits for anyway, issues pass 2 and goes into the run loop;
// pass 2's answer is looked at in .Lw_commit, where it has long arrived.  Its live lanes are not known yet, so the passes run
// over all 64 lanes: Dp is the set of lanes that share their hash with ANY lane of the window, restricted to the live lanes at
// the next head - a superset of the old one.  A lane that is in it only because of a dead partner resolves as before
// (.Lw_dup finds no kept / in-run lane -> .Lw_dupnone; the C++ loop does the same with a handed-back Dp).
//   v117 position of the next window's lanes   v116 / v115 what pass 1 / pass 2 read back   (the flush's scratch: the flush
//   runs at a window's end behind the commit and at an exit behind .Lw_x2, where these are dead)
// ORDER ON THE TABLE (the LDS returns and applies one wavefront's accesses in order):  between W's head and its commit the
// slots of W + 64's hashes hold positions of W + 64, not candidates, and nothing reads the table there: the run loop, .Lw_fix
// and .Lw_regather work on the cp register.  The roll-back (the slot's holder after pass 2 writes cpS = v159, which W's head
// read IN FRONT of pass 1) is the first LDS access of .Lw_commit, so it lies in front of the commit's own store (a slot both
// write keeps the commit's position), of the ip-2 put behind the commit (.Lw_pendset / S3S_ENGINE_PEND_NEXT), of the fresh table
// read of W + 64, of .Lw_cfix and of every hand-back at a window boundary (code 0) and every dispatch (sequential, skip, far,
// same): all of them see real candidates.  The one exit in mid-window (.Lw_x2, code 2) rolls back itself.  A window entered
// through .Lw_winm runs its own passes as before (the table is real then) and the next window's behind them.
// Needs the deferred emission (its register list has v115 - v117).  -DS3S_ENGINE_NO_DUP_AHEAD builds the round-6 head (A/B, tests).
#if defined(S3S_ENGINE_NO_DUP_AHEAD) || !defined(S3S_ENGINE_DEFER)
#undef S3S_ENGINE_DUP_AHEAD
#elif !defined(S3S_ENGINE_DUP_AHEAD)
#define S3S_ENGINE_DUP_AHEAD 1
#endif

// Layout (round 7): a taken branch costs ~25 cycles beyond its issue (profiles/r05_experiments.md §5) and the block's common
// paths were entered and left by one: same instructions, other order, chosen from the taken-branch column per label of
// tests/tools/chain_profile.py (profiles/lz4_chain.md §1 lists it before and after).
//  * .Lw_leave (the exit of 0.9 windows in 1.0) stands directly in front of the commit and falls into it; the rare .Lw_noev
//    (~50 per block) stands in front of it and jumps over it.
//  * .Lw_ext: the wait for the extension that is already in flight (.Lw_exth; 63 % of a TeraSort block's extensions) is the
//    fall-through and falls into the compare (.Lw_fwcmp); the on-demand extension (.Lw_extd) is the branch and jumps back.
//  * (ring) .Lw_extbr stands in line behind .Lw_extfull's ring issue and falls into .Lw_extbc2, see S3S_RING_EXTFULL.
// -DS3S_ENGINE_LAYOUT_R6 builds the round-6 order (A/B, tests).
#if defined(S3S_ENGINE_LAYOUT_R6)
#undef S3S_ENGINE_LAYOUT
#elif !defined(S3S_ENGINE_LAYOUT)
#define S3S_ENGINE_LAYOUT 1
#endif

// ---- THE INPUT RING (-DS3S_LZ4_RING: lz4_compress_ring_kernel, S3S_OPT_LZ4_VARIANT 11) ---------------------------------------
// The cooperative match extension is the last memory round trip on a window's chain (322 cycles alone, up to 1 180 behind other
// wavefronts' gathers; an LDS read is ~100).  With this macro the wavefront keeps the last 4 KiB of its input in LDS behind the
// table: the byte at chunk position q lies at LDS address 16384 + (q & 0xfff) (20 KiB per wavefront: eight per CU).
//  * RING WRITE.  The stream dwords D (256 bytes from wbase + 124, loaded two windows ahead) go into the ring when they have
//    arrived, at the end of the window's body; the one-window-skip and the far dispatch also write their D from wbase + 60.
//    Invariant in window W's run loop: the ring holds [W + 316 - 4096, W + 316) (from W's end on [W + 380 - 4096, W + 380)).
//    The ring's base is the DS offset field (no SGPR is left for it).
//  * ENTRY / RE-ENTRY.  Every entry into the block and every dispatch that is not sequential or a one-window skip passes
//    .Lw_dispf, which refills the ring from memory: the 4 KiB in front of W + 64 (four 1 KiB rows, addresses clamped at the
//    chunk's start: a slot whose position would be negative holds anything and is never read), then D from W + 60.
//  * VALIDITY.  "offset < S3S_RING_SPAN (3712)" is the whole test: the source side's aligned pairs start at src + 1 or later and
//    its backward bytes reach src - 64, both inside the ring for such an offset (ip >= W: src - 64 >= W - 3776 > W + 316 - 4096); the ip side lies in it by
//    construction.  AHEAD the ring holds 60 lanes' dwords (the pair of lane 59 ends at ip + 4 + 243 <= W + 63 + 247 < W + 316):
//    lanes 60..63 are made equal, so a match that runs through all 240 covered bytes takes the "no mismatch" exit (hand-back,
//    code 2: the C++ loop extends it from memory; with the global loads that exit is at 256 bytes, so matches of 244 .. 259
//    bytes from a near source are handed back now and cost a refill on re-entry: none in the benchmarked workloads, see
//    DESIGN.md section 6).  Any other offset takes the global loads unchanged.  The constants and the inequalities between them
//    stand next to S3S_RING_SPAN below, checked when the file is compiled.
//  * UNALIGNED READS.  A ds_read_b32 that is not dword-aligned is served lane by lane (65 cycles, tools/probe/lds_align_probe.hip)
//    and could not wrap; each side reads the ALIGNED PAIR around its dword instead (addresses masked per lane, so the ring's
//    wrap point needs neither a mirror margin nor a split read) and one v_alignbyte_b32 shifts it (the shift is the low two
//    bits of ip / of the candidate, taken by the instruction itself).
//  * THE EARLY ISSUE STAYS ON GLOBAL LOADS.  S3S_ENGINE_SPEC_COMMIT issues the next window's first extension while commit, table
//    read and dispatch run: its latency is off the chain already, and taking it from the ring put an LDS wait and ~18 instructions
//    ON the chain of every window (model: + 96 K cycles per TeraSort block against 118 K saved; measured: no gain, profiles/lz4_input_ring.md).  Only its
//    backward part (.Lw_extbx) comes from the ring.
//  * ORDER OF RETURNS.  LDS reads and global loads return independently, and an early extension the run loop passed by may still
//    be landing in v130 / v131: the ring path keeps its forward data in v150 / v151 (pairs' high dwords in v125 / v126, whose
//    role as load addresses ended at issue) and compares there.  Ring reads are always waited for (lgkmcnt(0)) at once.
#ifdef S3S_LZ4_RING
#if !defined(S3S_ENGINE_SPEC) || !defined(S3S_ENGINE_DEFER) || defined(S3S_ENGINE_PW_DIRECT) || defined(S3S_ENGINE_DLOAD_20)
#error "S3S_LZ4_RING is built on the shipped block (speculative gather, deferred emission, 64-lane stream load)"
#endif
#define S3S_RING_SPAN "0xe80"
/* the same constants as numbers, and what ties them together.  Assumptions: s76 (the window's base) is a multiple of 64 in chunk
   positions, so the ring's ds_write_b32 / ds_write_b128 are aligned to their width and no access straddles ring address 0xfff;
   an extension's ip is >= s76 (event lanes are lanes of the window); D reaches S3S_RING_AHEAD bytes behind s76 when the run loop
   of s76 runs (60 + 256, S3S_PW_DLOAD("60") / the previous window's S3S_PW_DLOAD("124")).
     behind: the lowest byte read is src - 64 (backward part) with src = ip - offset >= s76 - (SPAN - 1), and the ring's lowest
             position is s76 + AHEAD - BYTES:   SPAN - 1 + 64 + AHEAD <= BYTES   (3711 + 64 + 316 = 4091: five bytes to spare)
     ahead:  lane 59's aligned pair ends below ip + 4 + 4 * 59 + 8 <= s76 + 63 + 248:   63 + 248 <= AHEAD */
#define S3S_RING_BYTES 4096
#define S3S_RING_SPAN_N 0xe80
#define S3S_RING_AHEAD 316
#define S3S_RING_LANES 60
#if S3S_RING_SPAN_N - 1 + 64 + S3S_RING_AHEAD > S3S_RING_BYTES || 63 + 4 + 4 * (S3S_RING_LANES - 1) + 8 > S3S_RING_AHEAD
#error "S3S_RING_SPAN / S3S_RING_LANES no longer fit what the ring holds behind and ahead of a window"
#endif
#define S3S_RING_WRITE(OFF) /* v154 = D from s76 + OFF (v158 = s76 + 4 * lane) -> the ring */                 \
  "v_add_u32_e32 v158, " OFF ", v158\n\t"                                                                  \
  "v_and_b32_e32 v158, 0xfff, v158\n\t"                                                                    \
  "ds_write_b32 v158, v154 offset:16384\n\t"
#define S3S_RING_FILL_ISSUE /* the 4 KiB in front of s76 + 64: lane L takes 16 bytes of each 1 KiB row */      \
  "v_lshl_add_u32 v150, v129, 4, s76\n\t"                                                                  \
  "v_add_u32_e32 v151, 0xfffff040, v150\n\t"                                                               \
  "v_add_u32_e32 v152, 0xfffff440, v150\n\t"                                                               \
  "v_add_u32_e32 v153, 0xfffff840, v150\n\t"                                                               \
  "v_add_u32_e32 v150, 0xfffffc40, v150\n\t"                                                               \
  "v_max_i32_e32 v151, 0, v151\n\t"                                                                        \
  "v_max_i32_e32 v152, 0, v152\n\t"                                                                        \
  "v_max_i32_e32 v153, 0, v153\n\t"                                                                        \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  "global_load_dwordx4 v[168:171], v151, %[inp]\n\t"                                                       \
  "global_load_dwordx4 v[172:175], v152, %[inp]\n\t"                                                       \
  "global_load_dwordx4 v[176:179], v153, %[inp]\n\t"                                                       \
  "global_load_dwordx4 v[180:183], v150, %[inp]\n\t"
#define S3S_RING_FILL_WRITE /* (after vmcnt(0)) */                                                            \
  "v_lshl_add_u32 v150, v129, 4, s76\n\t"                                                                  \
  "v_add_u32_e32 v151, 64, v150\n\t"                                                                       \
  "v_add_u32_e32 v152, 0x440, v150\n\t"                                                                    \
  "v_add_u32_e32 v153, 0x840, v150\n\t"                                                                    \
  "v_add_u32_e32 v150, 0xc40, v150\n\t"                                                                    \
  "v_and_b32_e32 v151, 0xfff, v151\n\t"                                                                    \
  "v_and_b32_e32 v152, 0xfff, v152\n\t"                                                                    \
  "v_and_b32_e32 v153, 0xfff, v153\n\t"                                                                    \
  "v_and_b32_e32 v150, 0xfff, v150\n\t"                                                                    \
  "ds_write_b128 v151, v[168:171] offset:16384\n\t"                                                        \
  "ds_write_b128 v152, v[172:175] offset:16384\n\t"                                                        \
  "ds_write_b128 v153, v[176:179] offset:16384\n\t"                                                        \
  "ds_write_b128 v150, v[180:183] offset:16384\n\t"
/* v125 / v126 = the byte positions of every lane's ip-side / source-side dword -> the aligned pairs (v150, v125) / (v151, v126) */
#define S3S_RING_ISSUE                                                                                        \
  "v_and_b32_e32 v150, 0xffc, v125\n\t"                                                                    \
  "v_add_u32_e32 v125, 4, v125\n\t"                                                                        \
  "v_and_b32_e32 v151, 0xffc, v126\n\t"                                                                    \
  "v_add_u32_e32 v126, 4, v126\n\t"                                                                        \
  "v_and_b32_e32 v125, 0xffc, v125\n\t"                                                                    \
  "v_and_b32_e32 v126, 0xffc, v126\n\t"                                                                    \
  "ds_read_b32 v150, v150 offset:16384\n\t"                                                                \
  "ds_read_b32 v151, v151 offset:16384\n\t"                                                                \
  "ds_read_b32 v125, v125 offset:16384\n\t"                                                                \
  "ds_read_b32 v126, v126 offset:16384\n\t"
/* the pairs are back: shift (by the low two bits of ip = s89 / of the candidate = s88), lanes 60..63 equal; then the forward
   compare of .Lw_fwcmp / .Lw_extb on v150 / v151 (NOT v130 / v131: an early extension the run loop passed by may still be landing there) */
#define S3S_RING_FIN                                                                                          \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "s_lshr_b64 s[84:85], -1, 4\n\t"                                                                         \
  "v_alignbyte_b32 v150, v125, v150, s89\n\t"                                                              \
  "v_alignbyte_b32 v151, v126, v151, s88\n\t"                                                              \
  "v_cndmask_b32_e64 v151, v150, v151, s[84:85]\n\t"                                                       \
  "v_cmp_ne_u32_e64 s[82:83], v150, v151\n\t"
/* the backward bytes (up to 64 in front of ip and of the source) from the ring */
#define S3S_RING_BWD                                                                                          \
  "s_min_i32 s99, s92, s88\n\t"                                                                            \
  "v_mov_b32_e32 v127, 0\n\t"                                                                              \
  "v_mov_b32_e32 v128, 1\n\t"                                                                              \
  "v_cmp_gt_i32_e64 s[82:83], s99, v129\n\t"                                                               \
  "s_add_i32 s97, s89, -1\n\t"                                                                             \
  "s_add_i32 s98, s88, -1\n\t"                                                                             \
  "s_and_saveexec_b64 s[84:85], s[82:83]\n\t"                                                              \
  "v_sub_u32_e32 v123, s97, v129\n\t"                                                                      \
  "v_sub_u32_e32 v124, s98, v129\n\t"                                                                      \
  "v_and_b32_e32 v123, 0xfff, v123\n\t"                                                                    \
  "v_and_b32_e32 v124, 0xfff, v124\n\t"                                                                    \
  "ds_read_u8 v127, v123 offset:16384\n\t"                                                                 \
  "ds_read_u8 v128, v124 offset:16384\n\t"                                                                 \
  "s_mov_b64 exec, s[84:85]\n\t"
/* .Lw_ext, v125 / v126 / s98 = offset set: a source inside the span is served here, anything else falls through */
#define S3S_RING_EXT(NB)                                                                                      \
  "s_cmpk_lt_u32 s98, " S3S_RING_SPAN "\n\t"                                                               \
  "s_cbranch_scc0 .Lw_extg" NB "_%=\n\t"                                                                   \
  S3S_RING_ISSUE                                                                                           \
  "s_and_b32 s97, s87, 0xc00000\n\t"                                                                       \
  "s_cbranch_scc1 .Lw_mfullr" NB "_%=\n\t"                                                                 \
  ".Lw_fwonlyr" NB "_%=:\n\t"                                                                              \
  S3S_RING_FIN                                                                                             \
  "v_xor_b32_e32 v123, v150, v151\n\t"                                                                     \
  "s_branch .Lw_fwc2" NB "_%=\n\t"                                                                        \
  ".Lw_mfullr" NB "_%=:\n\t"                                                                               \
  "s_bitcmp1_b32 s87, 23\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_extbr" NB "_%=\n\t"                                                                  \
  "s_cmp_gt_i32 s92, 4\n\t"                                                                                \
  "s_cbranch_scc0 .Lw_fwonlyr" NB "_%=\n\t"                                                                \
  S3S_RING_EXTBR_HERE(NB)                                                                                  \
  /* the early extension (global loads into v130 / v131: vmcnt(2), see .Lw_exth) needs its backward part */  \
  ".Lw_mfullx" NB "_%=:\n\t"                                                                               \
  "s_bitcmp1_b32 s87, 23\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_extbx" NB "_%=\n\t"                                                                  \
  "s_cmp_gt_i32 s92, 4\n\t"                                                                                \
  "s_cbranch_scc0 .Lw_exthw" NB "_%=\n\t"                                                                  \
  ".Lw_extbx" NB "_%=:\n\t"                                                                                \
  "s_sub_i32 s98, s89, s88\n\t"                                                                            \
  "s_cmpk_lt_u32 s98, " S3S_RING_SPAN "\n\t"                                                               \
  "s_cbranch_scc0 .Lw_extb" NB "_%=\n\t"                                                                   \
  S3S_RING_BWD                                                                                             \
  "s_waitcnt vmcnt(2) lgkmcnt(0)\n\t"                                                                      \
  "s_branch .Lw_extbc" NB "_%=\n\t"                                                                        \
  ".Lw_extg" NB "_%=:\n\t"
#ifdef S3S_ENGINE_LAYOUT
/* (layout: .Lw_extbr is entered from .Lw_extfull - the duplicate-hash path - in 30 of 30 TeraSort and 276 of 277 wide-row
   visits per block: it stands in line there and falls into .Lw_extbc2; the global-load form of .Lw_extfull / .Lw_extb is the
   one that stands out of line, S3S_ENGINE_EXTB_OUTLINE) */
#define S3S_RING_EXTBR_HERE(NB) "s_branch .Lw_extbr" NB "_%=\n\t"
#define S3S_RING_EXTFULL(NB)                                                                                  \
  "s_cmpk_lt_u32 s98, " S3S_RING_SPAN "\n\t"                                                               \
  "s_cbranch_scc0 .Lw_extfg" NB "_%=\n\t"                                                                  \
  S3S_RING_ISSUE                                                                                           \
  ".Lw_extbr" NB "_%=:\n\t"                                                                                \
  S3S_RING_BWD                                                                                             \
  S3S_RING_FIN                                                                                             \
  "v_cmp_ne_u32_e64 s[84:85], v127, v128\n\t"                                                              \
  "v_xor_b32_e32 v123, v150, v151\n\t"
#define S3S_RING_EXTFG(NB) ".Lw_extfg" NB "_%=:\n\t"
#else
#define S3S_RING_EXTBR_HERE(NB)                                                                               \
  ".Lw_extbr" NB "_%=:\n\t"                                                                                \
  S3S_RING_BWD                                                                                             \
  S3S_RING_FIN                                                                                             \
  "v_cmp_ne_u32_e64 s[84:85], v127, v128\n\t"                                                              \
  "v_xor_b32_e32 v123, v150, v151\n\t"                                                                     \
  "s_branch .Lw_extbc2" NB "_%=\n\t"
#define S3S_RING_EXTFULL(NB)                                                                                  \
  "s_cmpk_lt_u32 s98, " S3S_RING_SPAN "\n\t"                                                               \
  "s_cbranch_scc0 .Lw_extfg" NB "_%=\n\t"                                                                  \
  S3S_RING_ISSUE                                                                                           \
  "s_branch .Lw_extbr" NB "_%=\n\t"                                                                        \
  ".Lw_extfg" NB "_%=:\n\t"
#define S3S_RING_EXTFG(NB)
#endif
#define S3S_RING_EXTBC(NB) ".Lw_extbc" NB "_%=:\n\t"
#define S3S_RING_EXTBC2(NB) ".Lw_extbc2" NB "_%=:\n\t"
#define S3S_RING_FWC2(NB) ".Lw_fwc2" NB "_%=:\n\t"
#define S3S_RING_EXTH_MFULL(NB) "s_cbranch_scc1 .Lw_mfullx" NB "_%=\n\t"
#define S3S_RING_EXTHW(NB) ".Lw_exthw" NB "_%=:\n\t"
#else
#define S3S_RING_WRITE(OFF)
#define S3S_RING_FILL_ISSUE
#define S3S_RING_FILL_WRITE
#define S3S_RING_EXT(NB)
#define S3S_RING_EXTFULL(NB)
#define S3S_RING_EXTFG(NB)
#define S3S_RING_EXTBC(NB)
#define S3S_RING_EXTBC2(NB)
#define S3S_RING_FWC2(NB)
#define S3S_RING_EXTH_MFULL(NB) "s_cbranch_scc1 .Lw_mfull" NB "_%=\n\t"
#define S3S_RING_EXTHW(NB)
#endif

#ifdef S3S_ENGINE_ABL_NOSTORE  // timing experiment only (wrong output): what do the sequence stores cost?
#define S3S_ENGINE_STORE ""
#else
#define S3S_ENGINE_STORE "global_store_byte v124, v122, %[outp]\n\t"
#endif

// cache policy of the candidate gather and of the sequence stores (A/B on hardware: profiles/r03_experiments.md)
#ifdef S3S_ABL_CLAMP_FAR  // timing experiment only (wrong output): candidates further back than N bytes are read N bytes back
#define S3S_ENGINE_STR_(x) #x
#define S3S_ENGINE_STR(x) S3S_ENGINE_STR_(x)
#define S3S_ENGINE_ABL_CLAMP "v_add_u32_e32 v152, -" S3S_ENGINE_STR(S3S_ABL_CLAMP_FAR) ", v148\n\tv_max_i32_e32 v150, v150, v152\n\t"
#else
#define S3S_ENGINE_ABL_CLAMP ""
#endif
// timing experiments (same output): the stream load / the candidate gather issued twice (second copy into v[160:163],
// never read) — what does one more 64-lane access cost the vector memory pipeline?
#ifdef S3S_ABL_DUP_PW
#define S3S_ENGINE_ABL_DUP_PW "global_load_dwordx4 v[160:163], v148, %[inp] offset:124\n\t"
#else
#define S3S_ENGINE_ABL_DUP_PW ""
#endif
#ifdef S3S_ABL_DUP_GATHER
#define S3S_ENGINE_ABL_DUP_GATHER "global_load_dwordx4 v[160:163], v150, %[inp]\n\t"
#else
#define S3S_ENGINE_ABL_DUP_GATHER ""
#endif
// timing experiment (same output): the extension's ip-side load issued twice — what would taking it from the stream
// registers (no memory access) be worth?
#ifdef S3S_ABL_DUP_IPSIDE
#define S3S_ENGINE_ABL_DUP_IPSIDE "global_load_dword v160, v125, %[inp]\n\t"
#else
#define S3S_ENGINE_ABL_DUP_IPSIDE ""
#endif
#if defined(S3S_X_GATHER_NT)
#define S3S_ENGINE_GATHER_POL " nt"
#elif defined(S3S_X_GATHER_SC1)
#define S3S_ENGINE_GATHER_POL " sc1"
#else
#define S3S_ENGINE_GATHER_POL ""
#endif


// ---- the stream bytes of a window (16 bytes p-4 .. p+11 per lane) WITHOUT a 64-lane x 16-byte load ----------------
// Round 3 (profiles/r03_experiments.md): the vector-memory pipeline is the second limiter of this kernel — one more
// 64-lane dwordx4 per window costs 8 % — and the stream load asked for 1 KiB to get 80 new bytes.  Now lanes 0..19
// load the window's 80 bytes once (v154 = dwords D[0..19] from wbase - 4), five ds_bpermute_b32 (the LDS crossbar, no
// LDS memory) hand lane L the dwords D[L/4 .. L/4 + 4] and four v_alignbyte_b32 shift them by L % 4.  The work is
// spread over three windows so that nothing waits: D is loaded at the dispatch of window W for window W + 128, moved
// across lanes at the end of W's body (behind the next table read), aligned in the gather's shadow of window W + 64,
// where the registers become pw1.  Invariant at every body entry: pw0 valid, v120..v124 = the five dwords of pw1
// (permutes issued), v154 = D of pw2 (load issued).  -DS3S_ENGINE_PW_DIRECT restores the direct 16-byte loads.
#ifndef S3S_ENGINE_PW_DIRECT
#ifndef S3S_ENGINE_DLOAD_20
/* (round 5, r05p: all 64 lanes load — lanes 20..63 fetch the 176 bytes behind, two more cache lines the next windows want anyway,
   and the two exec switches per window are gone: wide rows + 3 %, TeraSort + 0; the block runs at least 448 bytes from the
   chunk's end and the load reaches 124 + 256 behind the window.  -DS3S_ENGINE_DLOAD_20: lanes 0..19 only) */
#define S3S_PW_DLOAD(OFF) /* v154 <- dwords of the window at s76 + OFF + 4 */                                \
  "v_lshl_add_u32 v158, v129, 2, s76\n\t"                                                                  \
  "global_load_dword v154, v158, %[inp] offset:" OFF "\n\t"
#else
#define S3S_PW_DLOAD(OFF) /* v154 <- dwords of the window at s76 + OFF + 4 (lanes 0..19) */                  \
  "v_lshl_add_u32 v158, v129, 2, s76\n\t"                                                                  \
  "s_mov_b64 exec, 0xfffff\n\t"                                                                            \
  "global_load_dword v154, v158, %[inp] offset:" OFF "\n\t"                                                \
  "s_mov_b64 exec, -1\n\t"
#endif
#define S3S_PW_PERM /* v120..v124 <- D[L/4 .. L/4 + 4] */                                                    \
  "ds_bpermute_b32 v120, v157, v154\n\t"                                                                   \
  "ds_bpermute_b32 v121, v157, v154 offset:4\n\t"                                                          \
  "ds_bpermute_b32 v122, v157, v154 offset:8\n\t"                                                          \
  "ds_bpermute_b32 v123, v157, v154 offset:12\n\t"                                                         \
  "ds_bpermute_b32 v124, v157, v154 offset:16\n\t"
#define S3S_PW_ALIGN(R0, R1, R2, R3)                                                                          \
  "v_alignbyte_b32 " R0 ", v121, v120, v129\n\t"                                                            \
  "v_alignbyte_b32 " R1 ", v122, v121, v129\n\t"                                                            \
  "v_alignbyte_b32 " R2 ", v123, v122, v129\n\t"                                                            \
  "v_alignbyte_b32 " R3 ", v124, v123, v129\n\t"
#endif

#ifdef S3S_ENGINE_PW_DIRECT
#define S3S_ENGINE_PW2_COMMON(X) "global_load_dwordx4 " X ", v148, %[inp] offset:124\n\t"
#define S3S_ENGINE_PW1_ALIGN(R0, R1, R2, R3)
#define S3S_ENGINE_PW2_PERM
#define S3S_ENGINE_PW2_EXIT(R0, R1, R2, R3)
#define S3S_ENGINE_PENDB_REGS(NB, X1)                                                                          \
  "s_cmpk_lt_i32 s97, 0xc0\n\t"                                                                            \
  "s_cbranch_scc0 .Lw_pendc" NB "_%=\n\t"                                                                  \
  "s_add_i32 s97, s97, -128\n\t"                                                                           \
  "v_readlane_b32 s98, " X1 ", s97\n\t"                                                                    \
  "s_branch .Lw_pendset" NB "_%=\n\t"
#define S3S_ENGINE_DISP_SKIP(X, Y, Z0, Z1, Z2, Z3)                                                             \
  "global_load_dwordx4 " X ", v148, %[inp] offset:60\n\t"                                                  \
  "global_load_dwordx4 " Y ", v148, %[inp] offset:124\n\t"
#define S3S_ENGINE_DISP_FAR(Y, Z)                                                                              \
  "global_load_dwordx4 " Y ", v148, %[inp] offset:60\n\t"                                                  \
  "global_load_dwordx4 " Z ", v148, %[inp] offset:124\n\t"                                                 \
  "global_load_dword %[vp], v148, %[inp] offset:-64\n\t"                                                   \
  "s_waitcnt vmcnt(0)\n\t"
#define S3S_ENGINE_DISP_SAME(Y, Z)                                                                             \
  "global_load_dword %[vp], v148, %[inp] offset:-64\n\t"                                                   \
  "s_waitcnt vmcnt(0)\n\t"
#define S3S_ENGINE_ENTRY_PK
#else
#define S3S_ENGINE_PW2_COMMON(X) S3S_PW_DLOAD("124")
#define S3S_ENGINE_PW1_ALIGN(R0, R1, R2, R3) S3S_PW_ALIGN(R0, R1, R2, R3)
#define S3S_ENGINE_PW2_PERM S3S_PW_PERM
/* leaving the block: pw2 exists only as D (or as permuted dwords when the ring condition failed): finish it */
#define S3S_ENGINE_PW2_EXIT(R0, R1, R2, R3)                                                                    \
  S3S_PW_PERM                                                                                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  S3S_PW_ALIGN(R0, R1, R2, R3)
/* ip-2 two windows ahead: those bytes are not in registers (one dword from memory; rare) */
#define S3S_ENGINE_PENDB_REGS(NB, X1)
/* one window skipped: the window to run (Z) exists as permuted dwords; the two behind it come fresh */
#define S3S_ENGINE_DISP_SKIP(X, Y, Z0, Z1, Z2, Z3)                                                             \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  S3S_PW_ALIGN(Z0, Z1, Z2, Z3)                                                                             \
  S3S_PW_DLOAD("60")                                                                                       \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  S3S_RING_WRITE("60")                                                                                     \
  S3S_PW_PERM                                                                                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  S3S_PW_DLOAD("124")
/* anything else: pw0 by a direct load (issued by the caller of this macro), pw1 and pw2 through D */
#define S3S_ENGINE_DISP_FAR(Y, Z)                                                                              \
  S3S_RING_FILL_ISSUE                                                                                      \
  "global_load_dword %[vp], v148, %[inp] offset:-64\n\t"                                                   \
  S3S_PW_DLOAD("60")                                                                                       \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  S3S_RING_FILL_WRITE                                                                                      \
  S3S_RING_WRITE("60")                                                                                     \
  S3S_PW_PERM                                                                                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  S3S_PW_DLOAD("124")
/* (the block is always entered through .Lw_dispf, see S3S_ENGINE_ENTRY_PK: this case cannot occur) */
#define S3S_ENGINE_DISP_SAME(Y, Z) S3S_ENGINE_DISP_FAR(Y, Z)
/* entry: the C++ side holds whole windows; the ring wants pw1 / pw2 in flight: take the "anything else" dispatch */
#define S3S_ENGINE_ENTRY_PK "s_add_i32 %[pk], s76, -1\n\t"
#endif

#define S3S_ENGINE_PUT(B)                                                                                     \
  "s_cmp_eq_u32 %[putp], 0\n\t"                                                                            \
  "s_cbranch_scc1 .Lw_noput" B "_%=\n\t"                                                                   \
  "s_mul_i32 s97, %[vput], s79\n\t"                                                                        \
  "s_lshr_b32 s97, s97, 18\n\t"                                                                            \
  "s_and_b32 s97, s97, 0x3ffe\n\t"                                                                         \
  "s_add_i32 s98, %[base], -2\n\t"                                                                         \
  "v_mov_b32_e32 v150, s97\n\t"                                                                            \
  "v_mov_b32_e32 v151, s98\n\t"                                                                            \
  "ds_write_b16 v150, v151\n\t"                                                                            \
  "s_mov_b32 %[putp], 0\n\t"                                                                               \
  ".Lw_noput" B "_%=:\n\t"

// window conditions for the window that contains %[base]: t0 <= 48 && wbase >= 64 && wbase <= len - 384, and room for
// what one window can emit through this block (at most 16 short sequences, 78 literals: < 256 bytes; the ring bounds
// both wbase and op by s96 = len - 384).  384 bytes from the end nothing this block does can meet the end of the
// chunk: a probe is at most wbase + 63, a short-form match ends at most 4 + 269 bytes behind it (< len - 48: neither
// matchlimit = len - 5 nor mflimit = len - 12 is in reach, so there is no "last literals" exit) and the extension's
// loads reach at most 263 bytes behind the probe.  The C++ window path (fast_limit = len - 224) and the general batch
// take the chunk's last windows with their own limits.
// Literals: t0 <= 48 is also what keeps them in registers — a run that comes in from the previous window started at
// anchor = wbase - t0, so the literals of a window's first sequence begin at most 48 bytes in front of it, inside vp
// (the v of window wbase - 64, which every dispatch path provides); later sequences start inside the window.
// (with S3S_ENGINE_SPEC the block stops one window earlier: a window also issues the first extension of the NEXT window,
// whose loads must stay inside the chunk as well)
#ifdef S3S_ENGINE_SPEC
#define S3S_ENGINE_TAIL_BYTES "448"
#else
#define S3S_ENGINE_TAIL_BYTES "384"
#endif
#define S3S_ENGINE_COND_RING(FAIL)                                                                          \
  "s_and_b32 s76, %[base], 0xffffffc0\n\t"                                                                 \
  "s_sub_i32 s97, 48, %[t0]\n\t"                                                                           \
  "s_sub_i32 s98, s96, s76\n\t"                                                                            \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "s_sub_i32 s98, s96, %[op]\n\t"                                                                          \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "s_cmp_lt_i32 s97, 0\n\t"                                                                                \
  "s_cbranch_scc1 " FAIL "\n\t"

#define S3S_ENGINE_COND(FAIL)                                                                                 \
  "s_and_b32 s76, %[base], 0xffffffc0\n\t"                                                                 \
  "s_sub_i32 s97, 48, %[t0]\n\t"                                                                           \
  "s_add_i32 s98, s76, -64\n\t"                                                                            \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "s_sub_i32 s98, %[len], s76\n\t"                                                                         \
  "s_add_i32 s98, s98, -" S3S_ENGINE_TAIL_BYTES "\n\t"                                                     \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "s_sub_i32 s98, %[len], %[op]\n\t"                                                                       \
  "s_add_i32 s98, s98, -256\n\t"                                                                           \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "s_cmp_lt_i32 s97, 0\n\t"                                                                                \
  "s_cbranch_scc1 " FAIL "\n\t"


// ---- the per-lane event record from the 16 gathered bytes G (candidate - 4 .. candidate + 11) and the stream bytes Y ----
// (C = the register holding the candidates; vcc = "candidate closer than 4 bytes to the start of the chunk"; result: %[info]
// and s[82:83] = lanes whose candidate matches; LIVE = "" (all lanes) or the instruction that restricts s[82:83] to live lanes)
#define S3S_ENGINE_INFO(Y0, Y1, Y2, Y3, G0, G1, G2, G3, C, LIVE)                                               \
  "v_alignbyte_b32 v150, " G1 ", " G0 ", " C "\n\t"                                                         \
  "v_xor_b32_e32 v151, " G2 ", " Y2 "\n\t"                                                                  \
  "v_xor_b32_e32 v152, " G3 ", " Y3 "\n\t"                                                                  \
  "v_cndmask_b32_e32 v150, " G1 ", v150, vcc\n\t"                                                           \
  "v_xor_b32_e32 v153, " G0 ", " Y0 "\n\t"                                                                  \
  "v_cmp_eq_u32_e64 s[82:83], v150, " Y1 "\n\t"                                                            \
  "v_ffbl_b32_e32 v151, v151\n\t"                                                                          \
  "v_ffbl_b32_e32 v152, v152\n\t"                                                                          \
  "v_ffbh_u32_e32 v153, v153\n\t"                                                                          \
  LIVE                                                                                                     \
  "v_or_b32_e32 v152, 32, v152\n\t"                                                                        \
  "v_min_u32_e32 v153, 32, v153\n\t"                                                                       \
  "v_min3_u32 v151, v151, v152, 64\n\t"                                                                    \
  "v_lshrrev_b32_e32 v151, 3, v151\n\t"                                                                    \
  "v_lshrrev_b32_e32 v153, 3, v153\n\t"                                                                    \
  "v_cndmask_b32_e64 v153, v153, 8, vcc\n\t"                                                               \
  "v_cndmask_b32_e64 v151, v151, 8, vcc\n\t"                                                               \
  "v_lshl_or_b32 v152, v153, 20, " C "\n\t"                                                                \
  "v_lshl_or_b32 v151, v151, 16, v152\n\t"                                                                 \
  "v_or_b32_e32 v151, 0x40000000, v151\n\t"                                                                \
  "v_cndmask_b32_e64 %[info], 0, v151, s[82:83]\n\t"

#define S3S_ENGINE_LIVE_AND "s_and_b64 s[82:83], s[82:83], s[74:75]\n\t"

/* run-loop state of a window (scalar work; s78 = first live lane) */
#define S3S_ENGINE_RUN_INIT                                                                                   \
  "s_mov_b64 %[K], 0\n\t"                                                                                  \
  "s_mov_b32 %[rs], s78\n\t"                                                                               \
  "s_mov_b32 %[pendq], -1\n\t"                                                                             \
  "s_sub_i32 s97, %[t0], s78\n\t"                                                                          \
  "s_add_i32 s97, s97, -2\n\t"                                                                             \
  "s_max_i32 s97, s97, 0\n\t"                                                                              \
  "s_lshr_b64 %[valid], -1, s97\n\t"                                                                       \
  "s_lshl_b64 s[80:81], -1, s78\n\t"                                                                       \
  "s_and_b64 s[80:81], s[80:81], %[valid]\n\t"

#ifndef S3S_ENGINE_SPEC
// ---- the window's fixed part: table candidates (read issued earlier), gather, duplicate-hash passes, event records ----
#define S3S_ENGINE_FIXED(NB, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)                            \
  ".Lw_winf" NB "_%=:\n\t"                                                                                 \
  "s_sub_i32 s78, %[base], s76\n\t"                                                                        \
  "v_cmp_le_u32_e64 s[74:75], s78, v129\n\t"                                                               \
  /* (only the live lanes matter from here to the end of the duplicate passes) */                          \
  "s_mov_b64 exec, s[74:75]\n\t"                                                                           \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "ds_read_u16 v151, v149\n\t"                                                                             \
  "s_waitcnt lgkmcnt(2)\n\t"                                                                               \
  "v_cmp_gt_u32_e32 vcc, 4, %[cp]\n\t" /* near0: kept in vcc until the event records are built */          \
  "v_add_u32_e32 v150, -4, %[cp]\n\t"                                                                      \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  S3S_ENGINE_ABL_CLAMP                                                                                     \
  "global_load_dwordx4 " G ", v150, %[inp]" S3S_ENGINE_GATHER_POL "\n\t"                                     \
  S3S_ENGINE_ABL_DUP_GATHER                                                                                \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_ne_u32_e64 s[82:83], v151, v148\n\t"                                                              \
  "s_mov_b64 exec, s[82:83]\n\t"                                                                           \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "s_mov_b64 exec, s[74:75]\n\t"                                                                           \
  "ds_read_u16 v151, v149\n\t"                                                                             \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_ne_u32_e64 s[84:85], v151, v148\n\t"                                                              \
  "s_or_b64 %[Dp], s[82:83], s[84:85]\n\t"                                                                 \
  "s_andn2_b64 exec, s[74:75], s[84:85]\n\t"                                                               \
  "ds_write_b16 v149, %[cp]\n\t"                                                                           \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  S3S_ENGINE_PW1_ALIGN(Z0, Z1, Z2, Z3)                                                                      \
  /* run-loop state: scalar work in the shadow of the gather */                                            \
  S3S_ENGINE_RUN_INIT                                                                                      \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  S3S_ENGINE_INFO(Y0, Y1, Y2, Y3, G0, G1, G2, G3, "%[cp]", S3S_ENGINE_LIVE_AND)                             \
  "s_or_b64 %[ED], s[82:83], %[Dp]\n\t"
/* the next window's table read (all lanes): h, the table address, the read */
#define S3S_ENGINE_NEXT_TABLE_READ(Z1)                                                                        \
  "v_mul_lo_u32 v150, " Z1 ", s79\n\t"                                                                     \
  "v_lshrrev_b32_e32 %[h], 19, v150\n\t"                                                                   \
  "v_lshlrev_b32_e32 v149, 1, %[h]\n\t"                                                                    \
  "ds_read_u16 %[cp], v149\n\t"
#define S3S_ENGINE_FIXED_MISS(NB, X0, X1, X2, X3, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)
#define S3S_ENGINE_WIN_ENTRY(NB) "s_branch .Lw_winf" NB "_%=\n\t"
#define S3S_ENGINE_SPEC_ENTRY
#define S3S_ENGINE_SPEC_DUP(NB)
#define S3S_ENGINE_SPEC_X2(NB)
#define S3S_ENGINE_SPEC_EXT(NB)
#define S3S_ENGINE_SPEC_EXTFULL(NB)
#define S3S_ENGINE_SPEC_FWCMP(NB)
#define S3S_ENGINE_SPEC_NOEV(NB)
#define S3S_ENGINE_SPEC_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)
#else
// ---- SPECULATIVE NEXT-WINDOW GATHER + FIRST-EXTENSION PREFETCH (round 5, DESIGN.md §6.1e) ------------------------------
// The candidate gather is the one memory round trip every window waits for, and on TeraSort records three of four
// sequences need a second one (the cooperative extension).  Both are taken off the window's chain here:
//  * window W issues the gather for window W + 64 at its head — with the table as it is BEFORE W's commit (cpS = v159) —
//    into the register set of the body that runs next (GN);
//  * at W's END (the data is back by then) the event records of W + 64 are built from it, and for the first live lane
//    with a matching candidate whose forward length is capped (it will need the extension) the extension's two loads
//    are issued at once: commit, table read, dispatch and the next head run while they fly (%[code] = that lane);
//  * when W + 64 starts (sequential dispatch: .Lw_winf), the fresh table read cp decides lane by lane: cp == cpS -> the
//    record stands; a lane whose slot W's commit changed is STALE: its record becomes 0x80000000 and the lane an event.
//    Only if the run loop actually reaches such a lane (.Lw_dup sees bit 31) is it repaired (.Lw_fix): the fresh
//    candidate is nearly always a position of W itself (what its commit inserted), whose 16 bytes are W's stream
//    registers X of lane cp - (wbase - 64) — four ds_bpermute_b32; otherwise the gather is repeated (.Lw_regather).
//  * the run loop finds the prefetched extension at .Lw_ext (event lane == %[code]) and only waits for it.
// A window entered any other way (skip, far dispatch, block entry: .Lw_win -> .Lw_winm) gathers as before.
//   v155 / v156  table address / hash of the NEXT window's positions (reused for its table read), v159 cpS
// Wait counts (loads return in order among themselves; stores are never waited for by count):
//   window end  [.. spec gather of the next window .. youngest = a store] -> vmcnt(1); a window without any sequence has
//               [D load, spec gather] -> vmcnt(0) (.Lw_noev with K == 0);
//   .Lw_exth    [ext a, ext b, D load of the dispatch, spec gather issued at the head (, stores)] -> vmcnt(2);
//   .Lw_winm    [D load, gather, next spec gather] -> vmcnt(1).
// With S3S_LZ4_RING the same counts hold: the ring paths issue LDS accesses only and wait for them with lgkmcnt(0) at once
// (every LDS wait of the block is lgkmcnt(0), so the ring's writes never change a count); the refill's four row loads go out
// in .Lw_dispf in front of the D load and are covered by that dispatch's vmcnt(0); the ring write at a window's end sits behind
// the window-end vmcnt(0), which is what makes D valid; .Lw_extbx (backward part of the early extension from the ring) keeps
// .Lw_exth's vmcnt(2) for the forward loads and adds lgkmcnt(0).
// With S3S_ENGINE_DUP_AHEAD the head has ONE LDS wait behind the fresh table read instead of two (cpS and pass 1 of the next
// window, lgkmcnt(0)); pass 2's read-back is issued there and waited for by the lgkmcnt(0) that opens .Lw_commit (or .Lw_x2) -
// or by a ring path's lgkmcnt(0) in between, which then returns it early: every LDS wait is still lgkmcnt(0), and no vmcnt
// changes (the next window's gather is issued at the same place in the order of the vector-memory accesses).  What may be in
// the table when, and why the roll-back is safe against the commit and the ip-2 put: "ORDER ON THE TABLE" at the top of the file.
#ifdef S3S_ENGINE_PW_DIRECT
#error "S3S_ENGINE_SPEC needs the permuted stream load"
#endif
/* live lanes; the next window's stream bytes, hash, table address; its speculative table read; duplicate pass 1 */
#define S3S_SPEC_HEAD(Z0, Z1, Z2, Z3, STALE)                                                                   \
  "s_sub_i32 s78, %[base], s76\n\t"                                                                        \
  "v_cmp_le_u32_e64 s[74:75], s78, v129\n\t"                                                               \
  "s_waitcnt lgkmcnt(0)\n\t" /* cp of this window, the permuted stream dwords of the next */               \
  S3S_ENGINE_PW1_ALIGN(Z0, Z1, Z2, Z3)                                                                      \
  "v_mul_lo_u32 v155, " Z1 ", s79\n\t"                                                                     \
  STALE                                                                                                    \
  "v_lshrrev_b32_e32 v156, 19, v155\n\t"                                                                   \
  "v_lshlrev_b32_e32 v155, 1, v156\n\t"                                                                    \
  "ds_read_u16 v159, v155\n\t" /* cpS of the next window: the table before this window's passes and commit */\
  "s_mov_b64 exec, s[74:75]\n\t"                                                                           \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "ds_read_u16 v128, v149\n\t"
#define S3S_SPEC_PASS2_AND_NEXT_GATHER(GN)                                                                    \
  "s_waitcnt lgkmcnt(0)\n\t" /* pass 1 back, cpS of the next window back */                                \
  "v_cmp_ne_u32_e64 %[Dp], v128, v148\n\t"                                                                 \
  /* (the compare's result reaches the scalar unit ~25 cycles later: the next window's gather goes out in between) */\
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "v_add_u32_e32 v150, -4, v159\n\t"                                                                       \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  "global_load_dwordx4 " GN ", v150, %[inp]" S3S_ENGINE_GATHER_POL "\n\t"                                    \
  "s_mov_b64 exec, %[Dp]\n\t"                                                                              \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "s_mov_b64 exec, s[74:75]\n\t"                                                                           \
  "ds_read_u16 v128, v149\n\t" /* (exec stays on the live lanes until the second pass has been looked at) */ \
  S3S_ENGINE_RUN_INIT
#define S3S_SPEC_PASS2_DONE(FILL)                                                                             \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_ne_u32_e64 s[84:85], v128, v148\n\t" /* (live lanes: exec) */                                     \
  FILL                                                                                                     \
  "s_or_b64 %[Dp], %[Dp], s[84:85]\n\t"                                                                    \
  "s_andn2_b64 exec, s[74:75], s[84:85]\n\t"                                                               \
  "ds_write_b16 v149, %[cp]\n\t"                                                                           \
  "s_mov_b64 exec, -1\n\t"
#ifdef S3S_ENGINE_DUP_AHEAD
/* the next window's passes (all 64 lanes, exec = -1): pass 1 goes out behind the speculative table read ... */
#define S3S_DUPA_PASS1                                                                                        \
  "v_add_u32_e32 v117, 64, v148\n\t"                                                                       \
  "ds_write_b16 v155, v117\n\t"                                                                            \
  "ds_read_u16 v116, v155\n\t"
/* ... pass 2 when it is back (s[84:85] = the lanes that lost pass 1); nobody waits for v115 before .Lw_commit / .Lw_x2 */
#define S3S_DUPA_PASS2                                                                                        \
  "s_mov_b64 exec, s[84:85]\n\t"                                                                           \
  "ds_write_b16 v155, v117\n\t"                                                                            \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "ds_read_u16 v115, v155\n\t"
/* the roll-back: whoever holds a slot after pass 2 puts back what the head read in front of pass 1 (leaves exec = those lanes
   = vcc; "ORDER ON THE TABLE" at the top of the file) */
#define S3S_DUPA_ROLLBACK /* (after lgkmcnt(0)) */                                                            \
  "v_cmpx_eq_u32_e32 vcc, v115, v117\n\t"                                                             \
  "ds_write_b16 v155, v159\n\t"
/* sequential entry: the records were built at the end of the previous window, and so was Dp (all lanes: .Lw_commit) */
#define S3S_ENGINE_FIXED(NB, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)                            \
  ".Lw_winf" NB "_%=:\n\t"                                                                                 \
  "s_sub_i32 s78, %[base], s76\n\t"                                                                        \
  "v_cmp_le_u32_e64 s[74:75], s78, v129\n\t"                                                               \
  "s_waitcnt lgkmcnt(0)\n\t" /* cp of this window, the permuted stream dwords of the next */               \
  S3S_ENGINE_PW1_ALIGN(Z0, Z1, Z2, Z3)                                                                      \
  "v_mul_lo_u32 v155, " Z1 ", s79\n\t"                                                                     \
  "v_cmp_ne_u32_e64 vcc, %[cp], v159\n\t" /* stale lanes */                                                \
  "v_lshrrev_b32_e32 v156, 19, v155\n\t"                                                                   \
  "v_lshlrev_b32_e32 v155, 1, v156\n\t"                                                                    \
  "ds_read_u16 v159, v155\n\t" /* cpS of the next window: the table before its passes and this window's commit */\
  S3S_DUPA_PASS1                                                                                           \
  "s_mov_b64 exec, s[74:75]\n\t"                                                                           \
  "v_mov_b32_e32 v150, 0x80000000\n\t" /* (a literal next to vcc would be two constant-bus reads: not on gfx9) */ \
  "v_cndmask_b32_e32 %[info], %[info], v150, vcc\n\t" /* (live lanes only: exec) */                        \
  "v_cmp_ne_u32_e64 s[82:83], 0, %[info]\n\t" /* live lanes with a matching candidate, or stale */         \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "s_and_b64 %[Dp], %[Dp], s[74:75]\n\t"                                                                   \
  S3S_ENGINE_RUN_INIT                                                                                      \
  "s_waitcnt lgkmcnt(0)\n\t" /* cpS and pass 1 of the next window */                                       \
  "v_cmp_ne_u32_e64 s[84:85], v116, v117\n\t"                                                              \
  /* (the compare's result reaches the scalar unit ~25 cycles later: the next window's gather goes out in between) */\
  "v_add_u32_e32 v150, -4, v159\n\t"                                                                       \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  "global_load_dwordx4 " GN ", v150, %[inp]" S3S_ENGINE_GATHER_POL "\n\t"                                    \
  "s_or_b64 %[ED], s[82:83], %[Dp]\n\t"                                                                    \
  S3S_DUPA_PASS2
#define S3S_DUPA_MISS /* (the window's own passes are rolled back: the next window's, with a wait of their own) */ \
  S3S_DUPA_PASS1                                                                                           \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_ne_u32_e64 s[84:85], v116, v117\n\t"                                                              \
  S3S_DUPA_PASS2
#else
#define S3S_DUPA_MISS
/* sequential entry: the records were built at the end of the previous window */
#define S3S_ENGINE_FIXED(NB, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)                            \
  ".Lw_winf" NB "_%=:\n\t"                                                                                 \
  S3S_SPEC_HEAD(Z0, Z1, Z2, Z3, "v_cmp_ne_u32_e64 vcc, %[cp], v159\n\t") /* stale lanes */                    \
  "v_mov_b32_e32 v150, 0x80000000\n\t" /* (a literal next to vcc would be two constant-bus reads: not on gfx9) */ \
  "v_cndmask_b32_e32 %[info], %[info], v150, vcc\n\t" /* (live lanes only: exec) */                        \
  "v_cmp_ne_u32_e64 s[82:83], 0, %[info]\n\t" /* live lanes with a matching candidate, or stale */         \
  S3S_SPEC_PASS2_AND_NEXT_GATHER(GN)                                                                       \
  S3S_SPEC_PASS2_DONE("")                                                                                  \
  "s_or_b64 %[ED], s[82:83], %[Dp]\n\t"
#endif
#define S3S_SPEC_MISS_BODY(Z0, Z1, Z2, Z3, G, GN)                                                              \
  S3S_SPEC_HEAD(Z0, Z1, Z2, Z3, "")                                                                        \
  "v_cmp_gt_u32_e32 vcc, 4, %[cp]\n\t" /* near0: kept in vcc until the event records are built */          \
  "v_add_u32_e32 v150, -4, %[cp]\n\t"                                                                      \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  "global_load_dwordx4 " G ", v150, %[inp]" S3S_ENGINE_GATHER_POL "\n\t"                                     \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  S3S_SPEC_PASS2_AND_NEXT_GATHER(GN)                                                                       \
  S3S_SPEC_PASS2_DONE("")                                                                                  \
  S3S_DUPA_MISS
/* any other entry (out of line): gather with the fresh candidates, as without speculation */
#define S3S_ENGINE_FIXED_MISS(NB, X0, X1, X2, X3, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)       \
  ".Lw_winm" NB "_%=:\n\t"                                                                                 \
  S3S_SPEC_MISS_BODY(Z0, Z1, Z2, Z3, G, GN)                                                                 \
  "s_waitcnt vmcnt(1)\n\t"                                                                                 \
  ".Lw_info" NB "_%=:\n\t"                                                                                 \
  S3S_ENGINE_INFO(Y0, Y1, Y2, Y3, G0, G1, G2, G3, "%[cp]", S3S_ENGINE_LIVE_AND)                             \
  "s_or_b64 %[ED], s[82:83], %[Dp]\n\t"                                                                    \
  "s_branch .Lw_top" NB "_%=\n\t"                                                                          \
  /* a stale lane reached by the run loop: its fresh candidate is (nearly always) a position of the PREVIOUS window, */\
  /* whose 16 bytes are that window's stream registers X of lane cp - (wbase - 64) */                      \
  ".Lw_fix" NB "_%=:\n\t"                                                                                  \
  "v_cmp_gt_i32_e32 vcc, 0, %[info]\n\t" /* the placeholders = the stale lanes */                          \
  "s_add_i32 s97, s76, -64\n\t"                                                                            \
  "v_subrev_u32_e32 v150, s97, %[cp]\n\t"                                                                  \
  "v_cmp_gt_u32_e64 s[84:85], 64, v150\n\t"                                                                \
  "s_and_b64 s[84:85], s[84:85], vcc\n\t"                                                                  \
  "s_cmp_lt_u32 s76, 0x80\n\t" /* (window 64: the previous window's first lanes hold bytes from before the chunk) */\
  "s_cselect_b64 s[84:85], 0, s[84:85]\n\t"                                                                \
  "s_bitcmp1_b64 s[84:85], s86\n\t"                                                                        \
  "s_cbranch_scc0 .Lw_regather" NB "_%=\n\t"                                                               \
  "s_andn2_b64 s[72:73], vcc, s[84:85]\n\t" /* what stays stale */                                         \
  "v_lshlrev_b32_e32 v152, 2, v150\n\t"                                                                    \
  "ds_bpermute_b32 v120, v152, " X0 "\n\t"                                                                 \
  "ds_bpermute_b32 v121, v152, " X1 "\n\t"                                                                 \
  "ds_bpermute_b32 v122, v152, " X2 "\n\t"                                                                 \
  "ds_bpermute_b32 v123, v152, " X3 "\n\t"                                                                 \
  "v_cmp_gt_u32_e32 vcc, 4, %[cp]\n\t"                                                                     \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cndmask_b32_e64 " G0 ", " G0 ", v120, s[84:85]\n\t"                                                   \
  "v_cndmask_b32_e64 " G1 ", " G1 ", v121, s[84:85]\n\t"                                                   \
  "v_cndmask_b32_e64 " G2 ", " G2 ", v122, s[84:85]\n\t"                                                   \
  "v_cndmask_b32_e64 " G3 ", " G3 ", v123, s[84:85]\n\t"                                                   \
  S3S_ENGINE_INFO(Y0, Y1, Y2, Y3, G0, G1, G2, G3, "%[cp]", S3S_ENGINE_LIVE_AND)                             \
  "s_or_b64 %[ED], s[82:83], %[Dp]\n\t"                                                                    \
  "s_mov_b64 vcc, s[72:73]\n\t"                                                                            \
  "v_mov_b32_e32 v150, 0x80000000\n\t"                                                                     \
  "s_or_b64 %[ED], %[ED], s[72:73]\n\t"                                                                    \
  "v_cndmask_b32_e32 %[info], %[info], v150, vcc\n\t"                                                      \
  "s_branch .Lw_top" NB "_%=\n\t"                                                                          \
  /* ... or a hand-back while placeholders exist, or a candidate elsewhere: repeat the gather */           \
  ".Lw_regather" NB "_%=:\n\t"                                                                             \
  "v_cmp_gt_u32_e32 vcc, 4, %[cp]\n\t"                                                                     \
  "v_add_u32_e32 v150, -4, %[cp]\n\t"                                                                      \
  "v_max_i32_e32 v150, 0, v150\n\t"                                                                        \
  "global_load_dwordx4 " G ", v150, %[inp]" S3S_ENGINE_GATHER_POL "\n\t"                                     \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  "s_branch .Lw_info" NB "_%=\n\t"                                                                         \
  S3S_ENGINE_NVW(NB)
#define S3S_ENGINE_NEXT_TABLE_READ(Z1) /* (h was moved in the commit's shadow) */                            \
  "v_mov_b32_e32 v149, v155\n\t"                                                                           \
  "ds_read_u16 %[cp], v149\n\t"
#define S3S_ENGINE_WIN_ENTRY(NB) "s_branch .Lw_winm" NB "_%=\n\t"
#define S3S_ENGINE_SPEC_ENTRY "s_mov_b32 %[code], -1\n\t"
/* a stale lane reached by the run loop (its record has bit 31) */
#define S3S_ENGINE_SPEC_DUP(NB)                                                                               \
  "s_cmp_lt_i32 s87, 0\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_fix" NB "_%=\n\t"
/* handing back in mid-window: the C++ loop reads every lane's record, so they must all be real */
#define S3S_ENGINE_SPEC_X2(NB)                                                                                \
  "v_cmp_gt_i32_e32 vcc, 0, %[info]\n\t"                                                                   \
  "s_cmp_lg_u64 vcc, 0\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_regather" NB "_%=\n\t"
/* .Lw_ext: is this the extension that is already in flight? (any other extension overwrites its registers) */
#define S3S_ENGINE_SPEC_EXT(NB)                                                                               \
  "s_cmp_eq_u32 s86, %[code]\n\t"                                                                          \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_exth" NB "_%=\n\t"
#define S3S_ENGINE_SPEC_EXTFULL(NB) "s_mov_b32 %[code], -1\n\t"
#define S3S_ENGINE_SPEC_FWCMP(NB) ".Lw_fwcmp" NB "_%=:\n\t"
/* .Lw_noev: scc = (K != 0) = a sequence was emitted in this window */
#ifdef S3S_ENGINE_DEFER /* no sequence stores in the run loop: the next window's gather is always the youngest access */
#define S3S_ENGINE_SPEC_NOEV(NB)
#define S3S_ENGINE_NVW(NB)
#define S3S_ENGINE_WEND_VMCNT "s_waitcnt vmcnt(0)\n\t"
#else
#define S3S_ENGINE_SPEC_NOEV(NB)                                                                              \
  "s_cbranch_scc0 .Lw_nvw" NB "_%=\n\t"                                                                    \
  ".Lw_nvb" NB "_%=:\n\t"
#define S3S_ENGINE_WEND_VMCNT "s_waitcnt vmcnt(1)\n\t"
/* a window without any sequence so far: nothing younger than the next window's gather is in flight */
#define S3S_ENGINE_NVW(NB)                                                                                    \
  ".Lw_nvw" NB "_%=:\n\t"                                                                                  \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  "s_branch .Lw_nvb" NB "_%=\n\t"
#endif
/* which lane's extension is issued early: the first live lane with a matching candidate, if its record says "forward length
   capped".  (Taking the first live lane whose record says so instead — skipping short matches in front of it — found 53 % of the
   extensions in flight instead of 45 % and measured 1 % SLOWER: profiles/r05_experiments.md §5.) */
#define S3S_ENGINE_PF_MASK
#define S3S_ENGINE_PF_LANES "s[82:83]"
#define S3S_ENGINE_PF_CHECK(NB)                                                                               \
  "s_bitcmp1_b32 s99, 19\n\t"                                                                              \
  "s_cbranch_scc0 .Lw_nopf" NB "_%=\n\t"
/* window end, before the commit: the next window's records from its speculative gather (GN, cpS = v159, its stream bytes
   Z), and the extension of its first live matching lane when the record says it will need one */
#define S3S_ENGINE_SPEC_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)                                              \
  S3S_ENGINE_WEND_VMCNT                                                                                    \
  S3S_RING_WRITE("124")                                                                                    \
  "v_cmp_gt_u32_e32 vcc, 4, v159\n\t"                                                                      \
  S3S_ENGINE_INFO(Z0, Z1, Z2, Z3, N0, N1, N2, N3, "v159", "")                                               \
  S3S_ENGINE_PF_MASK                                                                                       \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  "s_sub_i32 s97, %[base], s76\n\t"                                                                        \
  "s_add_i32 s97, s97, -64\n\t" /* first live lane of the next window */                                   \
  "s_cmp_lt_u32 s97, 64\n\t"                                                                               \
  "s_cbranch_scc0 .Lw_nopf" NB "_%=\n\t"                                                                   \
  "s_lshr_b64 s[84:85], " S3S_ENGINE_PF_LANES ", s97\n\t"                                                  \
  "s_cbranch_scc0 .Lw_nopf" NB "_%=\n\t"                                                                   \
  "s_ff1_i32_b64 s98, s[84:85]\n\t"                                                                        \
  "s_add_i32 s98, s98, s97\n\t"                                                                            \
  "v_readlane_b32 s99, %[info], s98\n\t"                                                                   \
  "s_add_i32 s97, s76, s98\n\t" /* (in the shadow of the readlane) */                                      \
  S3S_ENGINE_PF_CHECK(NB)                                                                                  \
  "s_and_b32 s99, s99, 0xffff\n\t"                                                                         \
  "s_add_i32 s97, s97, 64\n\t" /* ip of that lane */                                                       \
  "s_sub_i32 s99, s97, s99\n\t" /* its offset */                                                           \
  "s_add_i32 s97, s97, 4\n\t"                                                                              \
  "v_lshl_add_u32 v125, v129, 2, s97\n\t"                                                                  \
  "v_subrev_u32_e32 v126, s99, v125\n\t"                                                                   \
  "global_load_dword v130, v125, %[inp]\n\t"                                                               \
  "global_load_dword v131, v126, %[inp]\n\t"                                                               \
  "s_mov_b32 %[code], s98\n\t"                                                                             \
  ".Lw_nopf" NB "_%=:\n\t"
#endif

// ---- commit: the highest kept lane of every hash group writes ----
#ifndef S3S_ENGINE_SPEC
#define S3S_ENGINE_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)                                                   \
  ".Lw_commit" NB "_%=:\n\t"                                                                                \
  "s_mov_b64 exec, %[K]\n\t"                                                                               \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "s_and_b64 s[82:83], %[K], %[Dp]\n\t"                                                                    \
  "s_bcnt1_i32_b64 s97, s[82:83]\n\t"                                                                      \
  "s_cmp_lt_u32 s97, 2\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_cdone" NB "_%=\n\t"                                                                  \
  ".Lw_cloop" NB "_%=:\n\t"                                                                                 \
  "ds_read_u16 v151, v149\n\t"                                                                             \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_lt_u32_e64 s[82:83], v151, v148\n\t"                                                              \
  "s_cmp_eq_u64 s[82:83], 0\n\t"                                                                           \
  "s_cbranch_scc1 .Lw_cdone" NB "_%=\n\t"                                                                  \
  "s_mov_b64 exec, s[82:83]\n\t"                                                                           \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "s_mov_b64 exec, %[K]\n\t"                                                                               \
  "s_branch .Lw_cloop" NB "_%=\n\t"                                                                        \
  ".Lw_cdone" NB "_%=:\n\t"                                                                                 \
  "s_mov_b64 exec, -1\n\t"
#define S3S_ENGINE_CFIX(NB)
#define S3S_ENGINE_PERM_AT_END S3S_ENGINE_PW2_PERM
#define S3S_DUPA_X2
#else
/* (round 5) the commit's store and its read-back go out FIRST; the next window's records and the extension prefetch are
   computed while that LDS round trip flies, and the compare's way to the scalar unit is covered by the stream permutes: the
   "did a lower position end up in a slot two kept lanes share" check used to be a round trip of its own in half the windows */
#ifdef S3S_ENGINE_DUP_AHEAD
/* the next window's passes are back: roll them back IN FRONT of the commit's store; Dp (dead in this window from here on: this
   commit does not look at it) becomes the next window's, over all 64 lanes: lost pass 1, or does not hold the slot after pass 2 */
#define S3S_DUPA_COMMIT_HEAD                                                                                  \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_ne_u32_e64 s[82:83], v116, v117\n\t" /* (all lanes: in front of the roll-back's exec) */          \
  S3S_DUPA_ROLLBACK
#define S3S_DUPA_COMMIT_DP "s_orn2_b64 %[Dp], s[82:83], vcc\n\t"
#define S3S_DUPA_X2                                                                                           \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  S3S_DUPA_ROLLBACK                                                                                        \
  "s_mov_b64 exec, -1\n\t"
#else
#define S3S_DUPA_COMMIT_HEAD
#define S3S_DUPA_COMMIT_DP
#define S3S_DUPA_X2
#endif
#define S3S_ENGINE_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)                                                   \
  ".Lw_commit" NB "_%=:\n\t"                                                                                \
  S3S_DUPA_COMMIT_HEAD                                                                                     \
  "s_mov_b64 exec, %[K]\n\t"                                                                               \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "ds_read_u16 v128, v149\n\t"                                                                             \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  S3S_DUPA_COMMIT_DP                                                                                       \
  S3S_ENGINE_SPEC_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)                                                \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "s_mov_b64 exec, %[K]\n\t"                                                                               \
  "v_cmp_lt_u32_e64 s[82:83], v128, v148\n\t"                                                              \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "v_mov_b32_e32 %[h], v156\n\t"                                                                           \
  S3S_ENGINE_PW2_PERM                                                                                      \
  "s_cmp_eq_u64 s[82:83], 0\n\t"                                                                           \
  "s_cbranch_scc0 .Lw_cfix" NB "_%=\n\t"                                                                   \
  ".Lw_cdone" NB "_%=:\n\t"
#define S3S_ENGINE_CFIX(NB)                                                                                   \
  ".Lw_cfix" NB "_%=:\n\t"                                                                                 \
  "s_mov_b64 exec, s[82:83]\n\t"                                                                           \
  "ds_write_b16 v149, v148\n\t"                                                                            \
  "s_mov_b64 exec, %[K]\n\t"                                                                               \
  "ds_read_u16 v128, v149\n\t"                                                                             \
  "s_waitcnt lgkmcnt(0)\n\t"                                                                               \
  "v_cmp_lt_u32_e64 s[82:83], v128, v148\n\t"                                                              \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "s_cmp_eq_u64 s[82:83], 0\n\t"                                                                           \
  "s_cbranch_scc0 .Lw_cfix" NB "_%=\n\t"                                                                   \
  "s_branch .Lw_cdone" NB "_%=\n\t"
#define S3S_ENGINE_PERM_AT_END
#endif

// the head of the run loop: next event lane, its record, the "same candidate as an earlier inserted lane" test
#if defined(S3S_ENGINE_TOP_R4) || defined(S3S_ENGINE_NO_SPEC)  /* the round-4 order (A/B) */
#define S3S_ENGINE_TOP(NB)                                                                                    \
  "s_ff1_i32_b64 s86, s[82:83]\n\t"                                                                        \
  "v_readlane_b32 s87, %[info], s86\n\t"                                                                   \
  "s_bitcmp0_b32 s87, 30\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_dup" NB "_%=\n\t"                                                                    \
  "s_and_b32 s88, s87, 0xffff\n\t"                                                                         \
  "v_cmp_eq_u32_e64 s[82:83], s88, %[cp]\n\t"                                                              \
  "s_or_b64 s[84:85], s[80:81], %[K]\n\t"                                                                  \
  "s_and_b64 s[82:83], s[82:83], s[84:85]\n\t"                                                             \
  "s_and_b64 s[82:83], s[82:83], %[Dp]\n\t"                                                                \
  "s_lshl_b64 s[84:85], -1, s86\n\t"                                                                       \
  "s_andn2_b64 s[82:83], s[82:83], s[84:85]\n\t"                                                           \
  "s_cbranch_scc1 .Lw_dup" NB "_%=\n\t"                                                                    \
  ".Lw_dkok" NB "_%=:\n\t"                                                                                 \
  "s_add_i32 s89, s76, s86\n\t"                                                                            \
  "s_bfe_u32 s90, s87, 0x40010\n\t"                                                                        \
  "s_bfe_u32 s91, s87, 0x30014\n\t"                                                                        \
  "s_sub_i32 s92, s89, %[anchor]\n\t"                                                                      \
  "s_min_i32 s91, s91, s92\n\t"
#else
#define S3S_ENGINE_TOP(NB)                                                                                    \
  "s_ff1_i32_b64 s86, s[82:83]\n\t"                                                                        \
  "v_readlane_b32 s87, %[info], s86\n\t"                                                                   \
  /* (round 5: a VALU result reaches the scalar unit ~25 cycles after its instruction issued — tools/probe/issue_probe.hip; */\
  /* what does not depend on the record or on the compare below is computed in those gaps: same instructions, other order) */\
  "s_add_i32 s89, s76, s86\n\t"                                                                            \
  "s_or_b64 s[84:85], s[80:81], %[K]\n\t"                                                                  \
  "s_sub_i32 s92, s89, %[anchor]\n\t"                                                                      \
  "s_lshl_b64 s[72:73], -1, s86\n\t"                                                                       \
  "s_bitcmp0_b32 s87, 30\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_dup" NB "_%=\n\t"                                                                    \
  "s_and_b32 s88, s87, 0xffff\n\t"                                                                         \
  "v_cmp_eq_u32_e64 s[82:83], s88, %[cp]\n\t"                                                              \
  "s_andn2_b64 s[84:85], s[84:85], s[72:73]\n\t"                                                           \
  "s_and_b64 s[84:85], s[84:85], %[Dp]\n\t"                                                                \
  "s_bfe_u32 s90, s87, 0x40010\n\t"                                                                        \
  "s_bfe_u32 s91, s87, 0x30014\n\t"                                                                        \
  "s_min_i32 s91, s91, s92\n\t"                                                                            \
  "s_and_b64 s[82:83], s[82:83], s[84:85]\n\t"                                                             \
  "s_cbranch_scc1 .Lw_dup" NB "_%=\n\t"                                                                    \
  ".Lw_dkok" NB "_%=:\n\t"
#endif

#ifdef S3S_ENGINE_DEFER
#define S3S_ENGINE_EMIT(Y1)                                                                                  \
  /* the sequence's record goes to lane m0 of v118 / v119; K, anchor as in the immediate form */           \
  "s_sub_i32 s98, s89, s88\n\t"                                                                            \
  "s_lshl4_add_u32 s97, s94, s93\n\t"                                                                      \
  "s_pack_ll_b32_b16 s98, s98, %[anchor]\n\t"                                                              \
  "v_writelane_b32 v119, s97, m0\n\t"                                                                      \
  "v_writelane_b32 v118, s98, m0\n\t"                                                                      \
  "s_lshl_b64 s[72:73], -2, s86\n\t"                                                                       \
  "s_andn2_b64 s[72:73], s[80:81], s[72:73]\n\t"                                                           \
  "s_add_i32 %[anchor], s89, 4\n\t"                                                                        \
  "s_or_b64 %[K], %[K], s[72:73]\n\t"                                                                      \
  "s_add_i32 %[anchor], %[anchor], s90\n\t"                                                                \
  "s_add_u32 m0, m0, 1\n\t"
#else
#define S3S_ENGINE_EMIT(Y1)                                                                                  \
  /* emit: token | literals (low bytes of v / vp) | offset | [match-length byte], one byte per lane */        \
  "v_subrev_u32_e32 v120, %[anchor], v129\n\t"                                                             \
  "s_min_i32 s97, s94, 15\n\t"                                                                             \
  "v_and_b32_e32 v120, 63, v120\n\t"                                                                       \
  "s_lshl4_add_u32 s97, s93, s97\n\t"                                                                      \
  "s_sub_i32 s98, s89, s88\n\t"                                                                            \
  "v_subrev_u32_e32 v121, s93, v120\n\t"                                                                   \
  "s_lshl_b32 s98, s98, 8\n\t"                                                                             \
  "v_add_u32_e32 v123, %[anchor], v120\n\t"                                                                \
  "s_or_b32 s97, s97, s98\n\t"                                                                             \
  "v_cmp_gt_i32_e32 vcc, s76, v123\n\t"                                                                    \
  "s_add_i32 s98, s94, -15\n\t"                                                                            \
  "s_lshl_b32 s98, s98, 24\n\t"                                                                            \
  "v_cndmask_b32_e32 v122, " Y1 ", %[vp], vcc\n\t"                                                         \
  "s_or_b32 s99, s97, s98\n\t"                                                                             \
  "v_lshlrev_b32_e32 v123, 3, v121\n\t"                                                                    \
  "v_lshrrev_b32_e64 v123, v123, s99\n\t"                                                                  \
  /* (the state update is interleaved: scalar instructions fill the wait states of the vcc consumers; anchor becomes ipe once its last reader has issued) */\
  "v_cmp_gt_u32_e32 vcc, s93, v120\n\t"                                                                    \
  "s_lshl_b64 s[72:73], -2, s86\n\t"                                                                       \
  "s_andn2_b64 s[72:73], s[80:81], s[72:73]\n\t"                                                           \
  "v_cndmask_b32_e32 v122, v123, v122, vcc\n\t"                                                            \
  "s_or_b64 %[K], %[K], s[72:73]\n\t"                                                                      \
  "s_add_i32 %[anchor], s89, 4\n\t"                                                                        \
  "v_addc_co_u32_e32 v124, vcc, 0, v120, vcc\n\t"                                                          \
  "v_cmp_ne_u32_e32 vcc, s93, v120\n\t"                                                                    \
  "v_cmp_gt_u32_e64 s[82:83], s95, v120\n\t"                                                               \
  "s_add_i32 %[anchor], %[anchor], s90\n\t"                                                                \
  "v_cndmask_b32_e32 v124, 0, v124, vcc\n\t"                                                               \
  "v_add_u32_e32 v124, %[op], v124\n\t"                                                                    \
  "s_and_saveexec_b64 s[84:85], s[82:83]\n\t"                                                              \
  S3S_ENGINE_STORE                                                                                         \
  "s_mov_b64 exec, s[84:85]\n\t"
#endif

// ---- deferred emission: the flush ------------------------------------------------------------------------------------
// m0 sequences wait in lanes 0 .. m0-1 of v118 (offset | anchor << 16) / v119 (literal length | match code << 4); they are
// consecutive in the output and end at %[op].  One lane per sequence: bytes = 1 token + lit (<= 14) + 2 offset + (1 if the
// match code is above 14) — 3 .. 18 bytes; a prefix sum places them, the literals come from memory (one 16-byte load per
// lane), the token goes in front (128-bit shift by one byte), offset and length byte are inserted behind the literals
// (64-bit shift into the dword pair that holds byte 1 + lit), and every lane stores exactly its bytes: whole dwords while
// they fit, then a halfword and a byte from the dword that holds the tail.  Called when more than 48 records wait at a
// window's end (a window adds at most 16: an event lane is at least 4 positions behind the previous one) and before the
// block hands back.  Clobbers v97 - v117, s[82:95], s97, vcc; s99 = the return site.  exec = -1 on entry and on return.
#ifdef S3S_ENGINE_DEFER
/* %[op] is brought up to date by the flush, not per sequence: inside the block it lags by the bytes of the waiting sequences
   (at most 64 x 18).  It is kept 1152 too HIGH instead, so that the ring's room check (op <= len - 448) stays on the safe side. */
#define S3S_ENGINE_DEFER_ENTRY "s_mov_b32 m0, 0\n\ts_add_i32 %[op], %[op], 0x480\n\t"
#define S3S_ENGINE_SEQ_BYTES
#define S3S_ENGINE_OP_ADVANCE
#define S3S_ENGINE_FLUSH_AT_WINDOW_END(NB)                                                                    \
  "s_cmp_gt_u32 m0, 48\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_flw" NB "_%=\n\t"                                                                    \
  ".Lw_frw" NB "_%=:\n\t"
#define S3S_ENGINE_FLUSH_AT_EXIT(NB)                                                                          \
  "s_cmp_eq_u32 m0, 0\n\t"                                                                                 \
  "s_cbranch_scc1 .Lw_frx" NB "_%=\n\t"                                                                    \
  "s_mov_b32 s99, 0x1" NB "\n\t"                                                                           \
  "s_branch .Lw_flush_%=\n\t"                                                                              \
  ".Lw_frx" NB "_%=:\n\t"                                                                                  \
  "s_add_i32 %[op], %[op], 0xfffffb80\n\t"
#define S3S_ENGINE_FLUSH_STUB(NB)                                                                             \
  ".Lw_flw" NB "_%=:\n\t"                                                                                  \
  "s_mov_b32 s99, " NB "\n\t"                                                                              \
  "s_branch .Lw_flush_%=\n\t"
#define S3S_ENGINE_FLUSH_DPP(CTRL)                                                                            \
  "s_nop 1\n\t"                                                                                            \
  "v_add_u32_dpp v100, v100, v100 " CTRL "\n\t"
#define S3S_ENGINE_FLUSH                                                                                      \
  ".Lw_flush_%=:\n\t"                                                                                      \
  "s_mov_b32 s86, m0\n\t"                                                                                  \
  "v_and_b32_e32 v97, 15, v119\n\t"            /* literal length */                                        \
  "v_lshrrev_b32_e32 v98, 4, v119\n\t"         /* match code = match length - 4 */                         \
  "v_cmp_gt_u32_e64 s[88:89], s86, v129\n\t"   /* lanes that hold a record */                              \
  "v_cmp_lt_u32_e32 vcc, 14, v98\n\t"                                                                      \
  "v_lshrrev_b32_e32 v102, 16, v118\n\t"       /* anchor */                                                \
  "v_and_b32_e32 v103, 0xffff, v118\n\t"       /* offset */                                                \
  "v_addc_co_u32_e32 v99, vcc, 3, v97, vcc\n\t"                                                            \
  "v_cndmask_b32_e64 v99, 0, v99, s[88:89]\n\t" /* bytes of the sequence */                                \
  "s_mov_b64 exec, s[88:89]\n\t"                                                                           \
  "global_load_dwordx4 v[104:107], v102, %[inp]\n\t"                                                       \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "v_mov_b32_e32 v100, v99\n\t"                                                                            \
  S3S_ENGINE_FLUSH_DPP("row_shr:1 row_mask:0xf bank_mask:0xf")                                             \
  S3S_ENGINE_FLUSH_DPP("row_shr:2 row_mask:0xf bank_mask:0xf")                                             \
  S3S_ENGINE_FLUSH_DPP("row_shr:4 row_mask:0xf bank_mask:0xf")                                             \
  S3S_ENGINE_FLUSH_DPP("row_shr:8 row_mask:0xf bank_mask:0xf")                                             \
  S3S_ENGINE_FLUSH_DPP("row_bcast:15 row_mask:0xa bank_mask:0xf")                                          \
  S3S_ENGINE_FLUSH_DPP("row_bcast:31 row_mask:0xc bank_mask:0xf")                                          \
  "v_add_u32_e32 v108, -15, v98\n\t"           /* the match-length byte */                                 \
  "v_readlane_b32 s87, v100, 63\n\t"           /* bytes of all waiting sequences */                        \
  "v_sub_u32_e32 v101, v100, v99\n\t"                                                                      \
  "v_lshl_or_b32 v108, v108, 16, v103\n\t"     /* tail = offset | length byte << 16 */                     \
  "v_mov_b32_e32 v109, 0\n\t"                                                                              \
  "v_add_u32_e32 v110, 1, v97\n\t"             /* the tail's byte position */                              \
  "s_add_i32 s97, %[op], 0xfffffb80\n\t"     /* where the first waiting sequence starts */               \
  "v_lshrrev_b32_e32 v111, 2, v110\n\t"        /* its dword */                                             \
  "v_and_b32_e32 v110, 3, v110\n\t"                                                                        \
  "v_add_u32_e32 v101, s97, v101\n\t"          /* where the lane's sequence starts in the output */        \
  "v_lshlrev_b32_e32 v110, 3, v110\n\t"                                                                    \
  "v_min_u32_e32 v115, 15, v98\n\t"                                                                        \
  "v_cmp_eq_u32_e64 s[90:91], 0, v111\n\t"                                                                 \
  "v_cmp_eq_u32_e64 s[92:93], 1, v111\n\t"                                                                 \
  "v_lshlrev_b64 v[112:113], v110, v[108:109]\n\t"                                                         \
  "v_bfm_b32 v114, v110, 0\n\t"                /* the bytes of that dword in front of the tail */          \
  "v_cmp_eq_u32_e64 s[94:95], 2, v111\n\t"                                                                 \
  "v_cmp_eq_u32_e64 s[82:83], 3, v111\n\t"                                                                 \
  "v_lshl_or_b32 v115, v97, 4, v115\n\t"       /* token */                                                 \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  "v_lshrrev_b32_e32 v116, 24, v107\n\t"       /* token | literals: the 16 loaded bytes one byte up */     \
  "v_alignbyte_b32 v107, v107, v106, 3\n\t"                                                                \
  "v_alignbyte_b32 v106, v106, v105, 3\n\t"                                                                \
  "v_alignbyte_b32 v105, v105, v104, 3\n\t"                                                                \
  "v_lshl_or_b32 v104, v104, 8, v115\n\t"                                                                  \
  "v_and_or_b32 v117, v104, v114, v112\n\t"    /* the tail goes into dword d (low part) and d + 1 */       \
  "v_cndmask_b32_e64 v104, v104, v117, s[90:91]\n\t"                                                       \
  "v_and_or_b32 v117, v105, v114, v112\n\t"                                                                \
  "v_cndmask_b32_e64 v105, v105, v117, s[92:93]\n\t"                                                       \
  "v_cndmask_b32_e64 v105, v105, v113, s[90:91]\n\t"                                                       \
  "v_and_or_b32 v117, v106, v114, v112\n\t"                                                                \
  "v_cndmask_b32_e64 v106, v106, v117, s[94:95]\n\t"                                                       \
  "v_cndmask_b32_e64 v106, v106, v113, s[92:93]\n\t"                                                       \
  "v_and_or_b32 v117, v107, v114, v112\n\t"                                                                \
  "v_cndmask_b32_e64 v107, v107, v117, s[82:83]\n\t"                                                       \
  "v_cndmask_b32_e64 v107, v107, v113, s[94:95]\n\t"                                                       \
  "v_cndmask_b32_e64 v116, v116, v113, s[82:83]\n\t"                                                       \
  /* whole dwords (lanes without a record have 0 bytes) */                                                 \
  "v_lshrrev_b32_e32 v108, 2, v99\n\t"         /* the dword that holds the last 1 - 3 bytes */             \
  "v_cmpx_le_u32_e32 vcc, 4, v99\n\t"                                                                      \
  "global_store_dword v101, v104, %[outp]\n\t"                                                             \
  "v_cmpx_le_u32_e32 vcc, 8, v99\n\t"                                                                      \
  "global_store_dword v101, v105, %[outp] offset:4\n\t"                                                    \
  "v_cmpx_le_u32_e32 vcc, 12, v99\n\t"                                                                     \
  "global_store_dword v101, v106, %[outp] offset:8\n\t"                                                    \
  "v_cmpx_le_u32_e32 vcc, 16, v99\n\t"                                                                     \
  "global_store_dword v101, v107, %[outp] offset:12\n\t"                                                   \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "v_cmp_eq_u32_e64 s[90:91], 3, v108\n\t"                                                                 \
  "v_cmp_eq_u32_e64 s[92:93], 2, v108\n\t"                                                                 \
  "v_cmp_eq_u32_e64 s[94:95], 1, v108\n\t"                                                                 \
  "v_cmp_eq_u32_e64 s[82:83], 0, v108\n\t"                                                                 \
  "v_and_b32_e32 v109, 28, v99\n\t"                                                                        \
  "v_cndmask_b32_e64 v116, v116, v107, s[90:91]\n\t"                                                       \
  "v_cndmask_b32_e64 v116, v116, v106, s[92:93]\n\t"                                                       \
  "v_cndmask_b32_e64 v116, v116, v105, s[94:95]\n\t"                                                       \
  "v_cndmask_b32_e64 v116, v116, v104, s[82:83]\n\t"                                                       \
  "v_add_u32_e32 v109, v101, v109\n\t"         /* address of the tail's dword */                           \
  "v_and_b32_e32 v110, 2, v99\n\t"                                                                         \
  "v_and_b32_e32 v111, 1, v99\n\t"                                                                         \
  "v_lshlrev_b32_e32 v112, 3, v110\n\t"                                                                    \
  "v_cmpx_ne_u32_e32 vcc, 0, v110\n\t"                                                                     \
  "global_store_short v109, v116, %[outp]\n\t"                                                             \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "v_add_u32_e32 v109, v109, v110\n\t"                                                                     \
  "v_lshrrev_b32_e32 v116, v112, v116\n\t"                                                                 \
  "v_cmpx_ne_u32_e32 vcc, 0, v111\n\t"                                                                     \
  "global_store_byte v109, v116, %[outp]\n\t"                                                              \
  "s_mov_b64 exec, -1\n\t"                                                                                 \
  "s_mov_b32 m0, 0\n\t"                                                                                    \
  "s_add_i32 %[op], %[op], s87\n\t"                                                                        \
  /* back to the site that asked (s99: 0 - 2 a window's end, 0x10 - 0x12 an exit, of body NB) */                 \
  "s_cmp_eq_u32 s99, 0\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_frw0_%=\n\t"                                                                         \
  "s_cmp_eq_u32 s99, 1\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_frw1_%=\n\t"                                                                         \
  "s_cmp_eq_u32 s99, 2\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_frw2_%=\n\t"                                                                         \
  "s_cmp_eq_u32 s99, 0x10\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_frx0_%=\n\t"                                                                         \
  "s_cmp_eq_u32 s99, 0x11\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_frx1_%=\n\t"                                                                         \
  "s_branch .Lw_frx2_%=\n\t"
#else
#define S3S_ENGINE_DEFER_ENTRY
#define S3S_ENGINE_SEQ_BYTES "s_cmp_gt_i32 s94, 14\n\ts_addc_u32 s95, s93, 3\n\t"
#define S3S_ENGINE_OP_ADVANCE "s_add_i32 %[op], %[op], s95\n\t"
#define S3S_ENGINE_FLUSH_AT_WINDOW_END(NB)
#define S3S_ENGINE_FLUSH_AT_EXIT(NB)
#define S3S_ENGINE_FLUSH_STUB(NB)
#define S3S_ENGINE_FLUSH
#endif


// LZ4_putPosition(ip - 2) when ip - 2 lies in the NEXT window (s97 = its distance to this window's base, 64 .. 127).
#ifdef S3S_ENGINE_SPEC
/* (round 5: that position's table address is lane s97 - 64 of v155 — the next window's hashes exist since this window's head —
   so one lane stores; before: its four bytes by v_readlane, the hash on the scalar unit, two v_mov, the store) */
#define S3S_ENGINE_PEND_NEXT(NB, Z1)                                                                          \
  "s_add_i32 s97, s97, -64\n\t"                                                                            \
  "v_mov_b32_e32 v151, %[pendq]\n\t"                                                                       \
  "s_lshl_b64 exec, 1, s97\n\t"                                                                            \
  "ds_write_b16 v155, v151\n\t"                                                                            \
  "s_mov_b64 exec, -1\n\t"
#define S3S_ENGINE_PEND_FAR(NB)                                                                               \
  "s_mul_i32 s98, s98, s79\n\t"                                                                            \
  "s_lshr_b32 s98, s98, 18\n\t"                                                                            \
  "s_and_b32 s98, s98, 0x3ffe\n\t"                                                                         \
  "v_mov_b32_e32 v150, s98\n\t"                                                                            \
  "v_mov_b32_e32 v151, %[pendq]\n\t"                                                                       \
  "ds_write_b16 v150, v151\n\t"                                                                            \
  "s_branch .Lw_nopend" NB "_%=\n\t"
#else
#define S3S_ENGINE_PEND_NEXT(NB, Z1)                                                                          \
  "s_add_i32 s97, s97, -64\n\t"                                                                            \
  "v_readlane_b32 s98, " Z1 ", s97\n\t"                                                                    \
  ".Lw_pendset" NB "_%=:\n\t"                                                                              \
  "s_mul_i32 s98, s98, s79\n\t"                                                                            \
  "s_lshr_b32 s98, s98, 18\n\t"                                                                            \
  "s_and_b32 s98, s98, 0x3ffe\n\t"                                                                         \
  "v_mov_b32_e32 v150, s98\n\t"                                                                            \
  "v_mov_b32_e32 v151, %[pendq]\n\t"                                                                       \
  "ds_write_b16 v150, v151\n\t"
#define S3S_ENGINE_PEND_FAR(NB) "s_branch .Lw_pendset" NB "_%=\n\t"
#endif

// ---- pieces of the run loop that S3S_ENGINE_LAYOUT places (same text in both orders) ----
/* the extension's load addresses: v125 = ip + 4 + 4 * lane, v126 = the same on the source side, s98 = offset */
#define S3S_ENGINE_EXT_ADDR                                                                                   \
  "s_add_i32 s97, s89, 4\n\t"                                                                              \
  "v_lshl_add_u32 v125, v129, 2, s97\n\t"                                                                  \
  "s_sub_i32 s98, s89, s88\n\t"                                                                            \
  "v_subrev_u32_e32 v126, s98, v125\n\t"
#define S3S_ENGINE_EXT_LOADS                                                                                  \
  "global_load_dword v130, v125, %[inp]\n\t"                                                               \
  S3S_ENGINE_ABL_DUP_IPSIDE                                                                                \
  "global_load_dword v131, v126, %[inp]\n\t"
/* the extension issued on demand, up to the arrival of its forward data (.Lw_fwcmp follows) */
#define S3S_ENGINE_EXT_ONDEMAND(NB)                                                                           \
  S3S_ENGINE_EXT_ADDR                                                                                      \
  S3S_RING_EXT(NB)                                                                                         \
  S3S_ENGINE_EXT_LOADS                                                                                     \
  "s_and_b32 s97, s87, 0xc00000\n\t"                                                                       \
  "s_cbranch_scc1 .Lw_mfull" NB "_%=\n\t"                                                                  \
  ".Lw_fwonly" NB "_%=:\n\t"                                                                               \
  "s_waitcnt vmcnt(0)\n\t"
/* the first extension of this window was issued at the end of the previous one: only wait for it (.Lw_fwcmp follows) */
#define S3S_ENGINE_EXT_EARLY(NB)                                                                              \
  ".Lw_exth" NB "_%=:\n\t"                                                                                 \
  "s_and_b32 s97, s87, 0xc00000\n\t"                                                                       \
  S3S_RING_EXTH_MFULL(NB)                                                                                  \
  S3S_RING_EXTHW(NB)                                                                                       \
  "s_waitcnt vmcnt(2)\n\t"
#if !defined(S3S_ENGINE_SPEC)
#define S3S_ENGINE_EXT_INLINE(NB) S3S_ENGINE_EXT_ONDEMAND(NB)
#define S3S_ENGINE_EXT_OUTLINE(NB)
#elif !defined(S3S_ENGINE_LAYOUT)
#define S3S_ENGINE_EXT_INLINE(NB)                                                                             \
  S3S_ENGINE_SPEC_EXT(NB)                                                                                  \
  S3S_ENGINE_EXT_ONDEMAND(NB)
#define S3S_ENGINE_EXT_OUTLINE(NB)                                                                            \
  S3S_ENGINE_EXT_EARLY(NB)                                                                                 \
  "s_branch .Lw_fwcmp" NB "_%=\n\t"
#else
/* .Lw_ext: is this the extension that is already in flight? (any other extension overwrites its registers) */
#define S3S_ENGINE_EXT_INLINE(NB)                                                                             \
  "s_cmp_eq_u32 s86, %[code]\n\t"                                                                          \
  "s_mov_b32 %[code], -1\n\t"                                                                              \
  "s_cbranch_scc0 .Lw_extd" NB "_%=\n\t"                                                                   \
  S3S_ENGINE_EXT_EARLY(NB)
#define S3S_ENGINE_EXT_OUTLINE(NB)                                                                            \
  ".Lw_extd" NB "_%=:\n\t"                                                                                 \
  S3S_ENGINE_EXT_ONDEMAND(NB)                                                                              \
  "s_branch .Lw_fwcmp" NB "_%=\n\t"
#endif
/* the backward part from memory (64 bytes in front of ip and of the source), the wait for both parts, the compares */
#define S3S_ENGINE_EXTB(NB)                                                                                   \
  ".Lw_extb" NB "_%=:\n\t"                                                                                 \
  "s_min_i32 s99, s92, s88\n\t"                                                                            \
  "v_mov_b32_e32 v127, 0\n\t"                                                                              \
  "v_mov_b32_e32 v128, 1\n\t"                                                                              \
  "v_cmp_gt_i32_e64 s[82:83], s99, v129\n\t"                                                               \
  "s_add_i32 s97, s89, -1\n\t"                                                                             \
  "s_add_i32 s98, s88, -1\n\t"                                                                             \
  "s_and_saveexec_b64 s[84:85], s[82:83]\n\t"                                                              \
  "v_sub_u32_e32 v123, s97, v129\n\t"                                                                      \
  "v_sub_u32_e32 v124, s98, v129\n\t"                                                                      \
  "global_load_ubyte v127, v123, %[inp]\n\t"                                                               \
  "global_load_ubyte v128, v124, %[inp]\n\t"                                                               \
  "s_mov_b64 exec, s[84:85]\n\t"                                                                           \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  S3S_RING_EXTBC(NB)                                                                                       \
  "v_cmp_ne_u32_e64 s[82:83], v130, v131\n\t"                                                              \
  "v_cmp_ne_u32_e64 s[84:85], v127, v128\n\t"                                                              \
  "v_xor_b32_e32 v123, v130, v131\n\t"
#if defined(S3S_LZ4_RING) && defined(S3S_ENGINE_LAYOUT)
#define S3S_ENGINE_EXTB_INLINE(NB)
#define S3S_ENGINE_EXTB_OUTLINE(NB)                                                                           \
  S3S_RING_EXTFG(NB)                                                                                       \
  S3S_ENGINE_EXT_LOADS                                                                                     \
  S3S_ENGINE_EXTB(NB)                                                                                      \
  "s_branch .Lw_extbc2" NB "_%=\n\t"
#else
#define S3S_ENGINE_EXTB_INLINE(NB)                                                                            \
  S3S_ENGINE_EXT_LOADS                                                                                     \
  S3S_ENGINE_EXTB(NB)
#define S3S_ENGINE_EXTB_OUTLINE(NB)
#endif
/* ---- the match left the window: ip-2 is either one of its last two lanes or goes to the next window ---- */
#define S3S_ENGINE_LEAVE(NB)                                                                                  \
  ".Lw_leave" NB "_%=:\n\t"                                                                                \
  "s_add_i32 s99, %[anchor], -2\n\t"                                                                       \
  "s_lshl_b64 s[82:83], 1, s98\n\t"                                                                        \
  "s_cmp_lt_i32 s98, 64\n\t"                                                                               \
  "s_cselect_b64 s[82:83], s[82:83], 0\n\t"                                                                \
  "s_cselect_b32 %[pendq], %[pendq], s99\n\t"                                                              \
  "s_or_b64 %[K], %[K], s[82:83]\n\t"                                                                      \
  "s_mov_b32 %[base], %[anchor]\n\t"                                                                       \
  "s_mov_b32 %[t0], 0\n\t"
#ifdef S3S_ENGINE_LAYOUT
#define S3S_ENGINE_LEAVE_R6(NB)
#define S3S_ENGINE_LEAVE_AT_COMMIT(NB)                                                                        \
  "s_branch .Lw_commit" NB "_%=\n\t"                                                                       \
  S3S_ENGINE_LEAVE(NB)
#else
#define S3S_ENGINE_LEAVE_R6(NB)                                                                               \
  S3S_ENGINE_LEAVE(NB)                                                                                     \
  "s_branch .Lw_commit" NB "_%=\n\t"
#define S3S_ENGINE_LEAVE_AT_COMMIT(NB)
#endif

// One step of the rotation: the dispatch for register roles B (X = bytes of window pk, Y = the next window, Z = the
// one after) followed by the window body for roles NB (pw0 = Y, pw1 = Z, pw2 = X), which the dispatch falls into
// when the window to run directly follows window pk.  NNB: the roles after a skipped window.  TAIL closes the ring.
#define S3S_ENGINE_STEP(B, NB, NNB, TAIL, X, X0, X1, X2, X3, XLO, XHI, Y, Y0, Y1, Y2, Y3, YLO, YHI, Z, Z0, Z1, Z2, \
                        Z3, ZLO, ZHI, G, G0, G1, G2, G3, GN, N0, N1, N2, N3)                                  \
  /* ---- dispatch: registers hold window pk, s76 = the window to run (conditions checked) ---- */           \
  ".Lw_disp" B "_%=:\n\t"                                                                                   \
  "v_add_u32_e32 v148, s76, v129\n\t"                                                                      \
  "s_sub_i32 s97, s76, %[pk]\n\t"                                                                          \
  "s_cmp_eq_u32 s97, 64\n\t"                                                                               \
  "s_cbranch_scc0 .Lw_dispx" B "_%=\n\t"                                                                   \
  "v_mov_b32_e32 %[vp], " X1 "\n\t"                                                                        \
  "s_mov_b32 %[pk], s76\n\t"                                                                               \
  S3S_ENGINE_PW2_COMMON(X)                                                                                 \
  S3S_ENGINE_ABL_DUP_PW                                                                                    \
  /* ---- the window: table candidates, gather, duplicate-hash passes, event records ---- */                 \
  /* (h, the table address and the table read of this window were issued at the end of the previous one, or by .Lw_win) */\
  S3S_ENGINE_FIXED(NB, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)                                    \
  /* ---- run loop: next event -> (one-round extension) -> short-form emit -> advance ---- */                \
  ".Lw_top" NB "_%=:\n\t"                                                                                  \
  "s_and_b64 s[82:83], s[80:81], %[ED]\n\t"                                                                \
  "s_cbranch_scc0 .Lw_noev" NB "_%=\n\t"                                                                   \
  S3S_ENGINE_TOP(NB)                                                                                       \
  "s_cmp_gt_i32 s92, 4\n\t"                                                                                \
  "s_cselect_b32 s97, 0x480000, s77\n\t"                                                                   \
  "s_and_b32 s97, s97, s87\n\t"                                                                            \
  "s_cbranch_scc0 .Lw_len" NB "_%=\n\t"                                                                    \
  /* cooperative extension, one round: 256 B forward; backward (64 B) only when the record's count is capped or unknown */\
  ".Lw_ext" NB "_%=:\n\t"                                                                                  \
  S3S_ENGINE_EXT_INLINE(NB)                                                                                \
  S3S_ENGINE_SPEC_FWCMP(NB)                                                                                \
  "v_cmp_ne_u32_e64 s[82:83], v130, v131\n\t"                                                              \
  "v_xor_b32_e32 v123, v130, v131\n\t"                                                                     \
  S3S_RING_FWC2(NB)                                                                                        \
  "s_cmp_eq_u64 s[82:83], 0\n\t"                                                                           \
  "s_cbranch_scc1 .Lw_x2" NB "_%=\n\t"                                                                     \
  "s_ff1_i32_b64 s98, s[82:83]\n\t"                                                                        \
  "v_readlane_b32 s90, v123, s98\n\t"                                                                      \
  "s_ff1_i32_b32 s90, s90\n\t"                                                                             \
  "s_lshr_b32 s90, s90, 3\n\t"                                                                             \
  "s_lshl2_add_u32 s90, s98, s90\n\t"                                                                      \
  /* lengths, short-form test */                                                                              \
  ".Lw_len" NB "_%=:\n\t"                                                                                   \
  "s_sub_i32 s93, s92, s91\n\t"                                                                            \
  "s_add_i32 s94, s91, s90\n\t"                                                                            \
  S3S_ENGINE_SEQ_BYTES                                                                                     \
  "s_add_i32 s97, s93, 0xff\n\t"                                                                           \
  "s_max_i32 s97, s97, s94\n\t"                                                                            \
  "s_cmpk_gt_i32 s97, 0x10d\n\t"                                                                           \
  "s_cbranch_scc1 .Lw_x2" NB "_%=\n\t"                                                                     \
  S3S_ENGINE_EMIT(Y1)                                                                                        \
  S3S_ENGINE_OP_ADVANCE                                                                                    \
  "s_sub_i32 %[rs], %[anchor], s76\n\t"                                                                    \
  "s_add_i32 s98, %[rs], -2\n\t"                                                                           \
  "s_cmp_lt_i32 %[rs], 64\n\t"                                                                             \
  "s_cbranch_scc0 .Lw_leave" NB "_%=\n\t"                                                                  \
  "s_bitset1_b64 %[K], s98\n\t"                                                                            \
  "s_lshl_b64 s[80:81], -1, %[rs]\n\t"                                                                     \
  "s_branch .Lw_top" NB "_%=\n\t"                                                                          \
  S3S_ENGINE_LEAVE_R6(NB)                                                                                  \
  /* ---- extension with the backward part ---- */                                                         \
  ".Lw_mfull" NB "_%=:\n\t"                                                                                \
  "s_bitcmp1_b32 s87, 23\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_extb" NB "_%=\n\t"                                                                   \
  "s_cmp_gt_i32 s92, 4\n\t"                                                                                \
  "s_cbranch_scc0 .Lw_fwonly" NB "_%=\n\t"                                                                 \
  "s_branch .Lw_extb" NB "_%=\n\t"                                                                         \
  ".Lw_extfull" NB "_%=:\n\t"                                                                              \
  S3S_ENGINE_SPEC_EXTFULL(NB)                                                                              \
  S3S_ENGINE_EXT_ADDR                                                                                      \
  S3S_RING_EXTFULL(NB)                                                                                     \
  S3S_ENGINE_EXTB_INLINE(NB)                                                                               \
  S3S_RING_EXTBC2(NB)                                                                                      \
  "s_ff1_i32_b64 s97, s[84:85]\n\t"                                                                        \
  "s_min_u32 s97, s97, 63\n\t"                                                                             \
  "s_cmp_eq_u32 s97, 63\n\t"                                                                               \
  "s_cbranch_scc1 .Lw_x2" NB "_%=\n\t"                                                                     \
  "s_cmp_eq_u64 s[82:83], 0\n\t"                                                                           \
  "s_cbranch_scc1 .Lw_x2" NB "_%=\n\t"                                                                     \
  "s_ff1_i32_b64 s98, s[82:83]\n\t"                                                                        \
  "v_readlane_b32 s90, v123, s98\n\t"                                                                      \
  "s_ff1_i32_b32 s90, s90\n\t"                                                                             \
  "s_lshr_b32 s90, s90, 3\n\t"                                                                             \
  "s_lshl2_add_u32 s90, s98, s90\n\t"                                                                      \
  ".Lw_got" NB "_%=:\n\t"                                                                                   \
  "s_mov_b32 s91, s97\n\t"                                                                                 \
  "s_branch .Lw_len" NB "_%=\n\t"                                                                          \
  /* ---- exact duplicate-hash resolution: the sequential code's candidate is the HIGHEST earlier lane of the window with */\
  /* the same hash that it has inserted (kept or in the current run), else the table candidate */          \
  ".Lw_dup" NB "_%=:\n\t"                                                                                  \
  S3S_ENGINE_SPEC_DUP(NB)                                                                                  \
  "v_readlane_b32 s88, %[h], s86\n\t"                                                                      \
  "s_or_b64 s[84:85], s[80:81], %[K]\n\t"                                                                  \
  "s_nop 0\n\t"                                                                                            \
  "v_cmp_eq_u32_e64 s[82:83], s88, %[h]\n\t"                                                               \
  "s_and_b64 s[82:83], s[82:83], s[84:85]\n\t"                                                             \
  "s_lshl_b64 s[84:85], -1, s86\n\t"                                                                       \
  "s_andn2_b64 s[82:83], s[82:83], s[84:85]\n\t"                                                           \
  "s_cbranch_scc0 .Lw_dupnone" NB "_%=\n\t"                                                                \
  "s_flbit_i32_b64 s97, s[82:83]\n\t"                                                                      \
  "s_sub_i32 s97, 63, s97\n\t"                                                                             \
  "v_readlane_b32 s98, " Y1 ", s97\n\t"                                                                    \
  "v_readlane_b32 s99, " Y1 ", s86\n\t"                                                                    \
  "s_cmp_eq_u32 s98, s99\n\t"                                                                              \
  "s_cbranch_scc0 .Lw_clear" NB "_%=\n\t"                                                                  \
  "s_add_i32 s88, s76, s97\n\t"                                                                            \
  "s_add_i32 s89, s76, s86\n\t"                                                                            \
  "s_sub_i32 s92, s89, %[anchor]\n\t"                                                                      \
  "s_branch .Lw_extfull" NB "_%=\n\t"                                                                          \
  ".Lw_dupnone" NB "_%=:\n\t"                                                                              \
  "s_bitcmp0_b32 s87, 30\n\t"                                                                              \
  "s_cbranch_scc1 .Lw_clear" NB "_%=\n\t"                                                                  \
  "s_and_b32 s88, s87, 0xffff\n\t"                                                                         \
  "s_branch .Lw_dkok" NB "_%=\n\t"                                                                         \
  ".Lw_clear" NB "_%=:\n\t"                                                                                \
  "s_lshl_b64 s[84:85], 1, s86\n\t"                                                                        \
  "s_andn2_b64 %[ED], %[ED], s[84:85]\n\t"                                                                 \
  "s_branch .Lw_top" NB "_%=\n\t"                                                                          \
  S3S_ENGINE_FIXED_MISS(NB, X0, X1, X2, X3, Y0, Y1, Y2, Y3, Z0, Z1, Z2, Z3, G, G0, G1, G2, G3, GN)               \
  S3S_ENGINE_EXT_OUTLINE(NB)                                                                               \
  S3S_ENGINE_EXTB_OUTLINE(NB)                                                                              \
  S3S_ENGINE_CFIX(NB)                                                                                      \
  S3S_ENGINE_FLUSH_STUB(NB)                                                                                \
  ".Lw_out0" NB "_%=:\n\t"                                                                                 \
  "s_mov_b32 %[code], 0\n\t"                                                                               \
  "s_branch .Lw_out" NB "_%=\n\t"                                                                          \
  ".Lw_x2" NB "_%=:\n\t"                                                                                    \
  S3S_ENGINE_SPEC_X2(NB)                                                                                   \
  S3S_DUPA_X2                                                                                              \
  "s_cmp_lg_u64 %[K], 0\n\t"                                                                               \
  "s_cselect_b64 %[valid], -1, %[valid]\n\t"                                                               \
  "s_mov_b32 %[code], 2\n\t"                                                                               \
  /* ---- leave: the stream registers go back to the C++ variables in window order ---- */                    \
  ".Lw_out" NB "_%=:\n\t"                                                                                   \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t"                                                                      \
  S3S_ENGINE_FLUSH_AT_EXIT(NB)                                                                             \
  S3S_ENGINE_PW2_EXIT(X0, X1, X2, X3)                                                                      \
  "s_add_i32 %[kp], %[pk], -64\n\t"                                                                        \
  "v_mov_b64 %[p0l], " YLO "\n\t"                                                                          \
  "v_mov_b64 %[p0h], " YHI "\n\t"                                                                          \
  "v_mov_b64 %[p1l], " ZLO "\n\t"                                                                          \
  "v_mov_b64 %[p1h], " ZHI "\n\t"                                                                          \
  "v_mov_b64 %[p2l], " XLO "\n\t"                                                                          \
  "v_mov_b64 %[p2h], " XHI "\n\t"                                                                          \
  "s_branch .Lw_end_%=\n\t"                                                                                \
  /* ---- ip-2 two windows ahead or further (rare) ---- */                                                 \
  ".Lw_pendb" NB "_%=:\n\t"                                                                                \
  S3S_ENGINE_PENDB_REGS(NB, X1)                                                                            \
  ".Lw_pendc" NB "_%=:\n\t"                                                                                \
  "v_mov_b32_e32 v151, %[pendq]\n\t"                                                                       \
  "global_load_dword v150, v151, %[inp]\n\t"                                                               \
  "s_waitcnt vmcnt(0)\n\t"                                                                                 \
  "v_readfirstlane_b32 s98, v150\n\t"                                                                      \
  S3S_ENGINE_PEND_FAR(NB)                                                                                  \
  /* ---- window entry without a table read in flight ---- */                                              \
  ".Lw_win" NB "_%=:\n\t"                                                                                  \
  "v_mul_lo_u32 v150, " Y1 ", s79\n\t"                                                                     \
  "v_lshrrev_b32_e32 %[h], 19, v150\n\t"                                                                   \
  "v_lshlrev_b32_e32 v149, 1, %[h]\n\t"                                                                    \
  "ds_read_u16 %[cp], v149\n\t"                                                                            \
  S3S_ENGINE_WIN_ENTRY(NB)                                                                                 \
  /* ---- dispatch, the other cases: same window again (entry only), one window skipped, anything else ---- */ \
  ".Lw_dispx" B "_%=:\n\t"                                                                                  \
  "s_cmp_eq_u32 s97, 0\n\t"                                                                                \
  "s_cbranch_scc1 .Lw_same" B "_%=\n\t"                                                                    \
  "s_cmpk_eq_u32 s97, 0x80\n\t"                                                                            \
  "s_cbranch_scc0 .Lw_dispf" B "_%=\n\t"                                                                   \
  "v_mov_b32_e32 %[vp], " Y1 "\n\t"                                                                        \
  "s_mov_b32 %[pk], s76\n\t"                                                                               \
  S3S_ENGINE_DISP_SKIP(X, Y, Z0, Z1, Z2, Z3)                                                               \
  "s_branch .Lw_win" NNB "_%=\n\t"                                                                         \
  ".Lw_dispf" B "_%=:\n\t"                                                                                  \
  "s_mov_b32 %[pk], s76\n\t"                                                                               \
  "global_load_dwordx4 " X ", v148, %[inp] offset:-4\n\t"                                                  \
  S3S_ENGINE_DISP_FAR(Y, Z)                                                                                \
  "s_branch .Lw_win" B "_%=\n\t"                                                                           \
  ".Lw_same" B "_%=:\n\t"                                                                                  \
  S3S_ENGINE_DISP_SAME(Y, Z)                                                                               \
  "s_branch .Lw_win" B "_%=\n\t"                                                                           \
  /* ---- the run leaves the window (or its consecutive part) without a match ---- */                         \
  ".Lw_noev" NB "_%=:\n\t"                                                                                  \
  "s_sub_i32 s97, s78, %[t0]\n\t"                                                                          \
  "s_add_i32 s97, s97, 66\n\t"                                                                             \
  "s_min_i32 s97, s97, 64\n\t"                                                                             \
  "s_cmp_lg_u64 %[K], 0\n\t"                                                                               \
  "s_cselect_b32 s97, 64, s97\n\t"                                                                         \
  "s_cselect_b32 s98, 0, %[t0]\n\t"                                                                        \
  S3S_ENGINE_SPEC_NOEV(NB)                                                                                 \
  "s_or_b64 %[K], %[K], s[80:81]\n\t"                                                                      \
  "s_add_i32 %[base], s76, s97\n\t"                                                                        \
  "s_add_i32 s98, s98, s97\n\t"                                                                            \
  "s_sub_i32 %[t0], s98, %[rs]\n\t"                                                                        \
  /* (a run that leaves its consecutive part comes out with t0 = 66: the ring condition below hands it to the general batch) */\
  S3S_ENGINE_LEAVE_AT_COMMIT(NB)                                                                           \
  /* ---- commit: the highest kept lane of every hash group writes ---- */                                    \
  S3S_ENGINE_COMMIT(NB, Z0, Z1, Z2, Z3, N0, N1, N2, N3)                                                    \
  /* ---- LZ4_putPosition(ip - 2) behind the window (its bytes are in the registers of the next two windows) ---- */\
  "s_cmp_lt_i32 %[pendq], 0\n\t"                                                                           \
  "s_cbranch_scc1 .Lw_nopend" NB "_%=\n\t"                                                                 \
  "s_sub_i32 s97, %[pendq], s76\n\t"                                                                       \
  "s_cmpk_lt_i32 s97, 0x80\n\t"                                                                            \
  "s_cbranch_scc0 .Lw_pendb" NB "_%=\n\t"                                                                  \
  S3S_ENGINE_PEND_NEXT(NB, Z1)                                                                             \
  ".Lw_nopend" NB "_%=:\n\t"                                                                                \
  /* the next window's table read goes out now (all lanes): it is back when the window condition and the dispatch are through */\
  S3S_ENGINE_NEXT_TABLE_READ(Z1)                                                                           \
  S3S_ENGINE_PERM_AT_END                                                                                      \
  S3S_ENGINE_COND_RING(".Lw_out0" NB "_%=")                                                                \
  S3S_ENGINE_FLUSH_AT_WINDOW_END(NB)                                                                       \
  TAIL

#define S3S_RA "v[132:135]", "v132", "v133", "v134", "v135", "v[132:133]", "v[134:135]"
#define S3S_RB "v[136:139]", "v136", "v137", "v138", "v139", "v[136:137]", "v[138:139]"
#define S3S_RC "v[140:143]", "v140", "v141", "v142", "v143", "v[140:141]", "v[142:143]"
#define S3S_ENGINE_STEP_(B, NB, NNB, TAIL, ...) S3S_ENGINE_STEP(B, NB, NNB, TAIL, __VA_ARGS__)
// gather register sets: body k builds its records from set k; with S3S_ENGINE_SPEC it has the next body's set filled
#define S3S_G0 "v[144:147]", "v144", "v145", "v146", "v147"
#ifdef S3S_ENGINE_SPEC
#define S3S_G1 "v[160:163]", "v160", "v161", "v162", "v163"
#define S3S_G2 "v[164:167]", "v164", "v165", "v166", "v167"
#define S3S_GR0 S3S_G0
#define S3S_GR1 S3S_G1
#define S3S_GR2 S3S_G2
#else
#define S3S_G1 S3S_G0
#define S3S_G2 S3S_G0
#define S3S_GR0 S3S_G0
#define S3S_GR1 S3S_G0
#define S3S_GR2 S3S_G0
#endif


#define S3S_WINDOW_ENGINE_ASM                                                                                 \
  "v_mbcnt_lo_u32_b32 v129, -1, 0\n\t"                                                                     \
  "v_mbcnt_hi_u32_b32 v129, -1, v129\n\t"                                                                  \
  "s_mov_b32 s79, 0x9e3779b1\n\t"                                                                          \
  "v_mov_b64 v[132:133], %[p0l]\n\t"                                                                       \
  "v_mov_b64 v[134:135], %[p0h]\n\t"                                                                       \
  "v_mov_b64 v[136:137], %[p1l]\n\t"                                                                       \
  "v_mov_b64 v[138:139], %[p1h]\n\t"                                                                       \
  "v_mov_b64 v[140:141], %[p2l]\n\t"                                                                       \
  "v_mov_b64 v[142:143], %[p2h]\n\t"                                                                       \
  "s_mov_b32 %[code], 0\n\t"                                                                               \
  "s_add_i32 s96, %[len], -" S3S_ENGINE_TAIL_BYTES "\n\t"                                                  \
  "s_mov_b32 s77, 0x80000\n\t"                                                                             \
  S3S_ENGINE_PUT("E")                                                                                      \
  S3S_ENGINE_COND(".Lw_end_%=")                                                                               \
  S3S_ENGINE_ENTRY_PK                                                                                      \
  S3S_ENGINE_SPEC_ENTRY                                                                                    \
  S3S_ENGINE_DEFER_ENTRY                                                                                   \
  "v_and_b32_e32 v157, 0xfc, v129\n\t"                                                                     \
  "v_mul_lo_u32 v150, v137, s79\n\t"                                                                       \
  "v_lshrrev_b32_e32 %[h], 19, v150\n\t"                                                                   \
  "v_lshlrev_b32_e32 v149, 1, %[h]\n\t"                                                                    \
  "ds_read_u16 %[cp], v149\n\t"                                                                            \
  S3S_ENGINE_STEP_("0", "1", "2", "", S3S_RA, S3S_RB, S3S_RC, S3S_G1, S3S_GR2)                                \
  S3S_ENGINE_STEP_("1", "2", "0", "", S3S_RB, S3S_RC, S3S_RA, S3S_G2, S3S_GR0)                                \
  S3S_ENGINE_STEP_("2", "0", "1", "s_branch .Lw_disp0_%=\n\t", S3S_RC, S3S_RA, S3S_RB, S3S_G0, S3S_GR1)       \
  S3S_ENGINE_FLUSH                                                                                         \
  ".Lw_end_%=:\n\t"
