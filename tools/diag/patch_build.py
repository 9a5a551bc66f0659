"""Timing-diagnostic builds of the library from PATCHED COPIES of csrc/ (never -D knobs in the
product sources): each diagnostic is a list of exact text substitutions applied to a copy of
deepinteract_amd/csrc + include/, built into deepinteract_amd/lib/variants/diag_<name>/ and loaded
with bench.py --lib. Every diagnostic computes WRONG results on purpose (timing only), except the
A/B variants marked as such (one-line launch / pipeline changes measured against the product).
Every pattern must occur in its file exactly `count` times (tests/test_diag_patches.py); a
diagnostic of code that has since been deleted is deleted with it (tools/diag/build_rev.py builds a
past tree).

usage: python tools/diag/patch_build.py nosilu nosync ringw0 initnopos initnostore initw0 ...
"""
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepinteract_amd import build  # noqa: E402

DIAGS = {
    # the edge layers' SiLU epilogues as a plain multiply (no transcendentals): how much of the step a
    # faster GeoT converts into throughput
    "nosilu": [("mfma32.h", "for (int k = 0; k < 16; ++k) v[k] = silu2<true>(v[k]);",
                "for (int k = 0; k < 16; ++k) v[k] = v[k] * 0.5f;", 1)],
    # the double-buffered weight stages switch without waiting for their LDS-DMA or a barrier
    "nosync": [("common.h", """    if constexpr (DBUF) {
      lds_dma_wait();
      __syncthreads();
      cur ^= 1;""", """    if constexpr (DBUF) {
      cur ^= 1;""", 1)],
    # InitEdge (k_init_x32) without the positional-table gathers: acc starts at zero
    "initnopos": [("geot_init.hip", "  init_acc_x32(acc, a, a.node_pos[a.src[e]], a.node_pos[a.dst[e]], h);\n  const bool with_fn",
                   "  zero(acc);\n  const bool with_fn", 1)],
    # InitEdge without its F row stores (kept alive by a never-true condition)
    "initnostore": [("geot_init.hip", "  store_f(f, a.f_out);\n  if (!with_fn) return;",
                     "  if (f.v[0][0] == 1.2345e30f) store_f(f, a.f_out);\n  if (!with_fn) return;", 1)],
    # InitEdge's weight phases all DMA'd from the blob's first blocks (L2-resident; wrong weights)
    "initw0": [("geot_init.hip", """    if (p == 0) pipe.issue(W + (IE_T0 + 40 * geo_t(0)) * BLK, 40);
    else if (p < NT) pipe.issue(W + (IE_T0 + 40 * geo_t(p)) * BLK, 40);
    else if (p == NT) {
      if constexpr (GC) {  // em1, dist1 and amide1 only: dir1 / orient1 (blocks 16-31) are never read
        pipe.issue(W + IE_GEO1 * BLK, 16);
        pipe.issue2(W + (IE_GEO1 + 32) * BLK, 8);
      } else {
        pipe.issue(W + IE_GEO1 * BLK, 40);
      }
    }
    else if (p == NT + 1) pipe.issue(W + IE_C1 * BLK, Z ? 8 : 16);""", """    if (p == 0) pipe.issue(W, 40);
    else if (p < NT) pipe.issue(W, 40);
    else if (p == NT) pipe.issue(W, GC ? 24 : 40);
    else if (p == NT + 1) pipe.issue(W, Z ? 8 : 16);""", 1)],
    # A/B variants with CORRECT results (timing comparisons of one-line changes, never shipped):
    # k_init_x32<true, *>'s gates phase fetching all 40 blocks of IE_GEO1 (dir1 / orient1 unread), as
    # before the 16 + 8 fetch: the arm of profiles/wide_rows_ab.txt that separates that change
    "gate40": [("geot_init.hip", """      if constexpr (GC) {  // em1, dist1 and amide1 only: dir1 / orient1 (blocks 16-31) are never read
        pipe.issue(W + IE_GEO1 * BLK, 16);
        pipe.issue2(W + (IE_GEO1 + 32) * BLK, 8);
      } else {""", """      if constexpr (false) {
      } else {""", 1),
               ("geot_init.hip", "  auto gate_off = [](int t) { return GC ? (t == 0 ? 0 : (t == 1 ? 8 : 16)) : 8 * t; };",
                "  auto gate_off = [](int t) { return 8 * t; };", 1)],
    # the edge ring issuing each weight stage three stages ahead (two in the product)
    "ahead3": [("geot_edge.hip", "constexpr int RING_NW = 8, RING_SLOTS = 4, RING_AHEAD = 2;",
                "constexpr int RING_NW = 8, RING_SLOTS = 4, RING_AHEAD = 3;", 1)],
    # InitEdge (k_init_x32) in 6-wave blocks, two per CU (four-wave blocks, three per CU, in the
    # product): 192 instead of 128 edges per weight pass
    "init6": [("geot_init.hip", "constexpr int INIT_X32_NW = 4;", "constexpr int INIT_X32_NW = 6;", 1)],
    # the persistent edge ring on 8 CUs fewer than the device has: room for a collective's blocks
    # beside it (the chunked gather's exposure)
    # (every launch of the ring, the z0 layer 0 included: launch_edge_ring)
    "ring248": [("geot_edge.hip", "  const PersistentGrid p = persistent_grid(a.Et, EdgeRingGeo::ROWS);",
                 "  PersistentGrid p = persistent_grid(a.Et, EdgeRingGeo::ROWS);\n"
                 "  if ((int)p.grid.x > device_cus() - 8) p.grid.x = (unsigned)(device_cus() - 8);", 1)],
    # k_node_ws's segment sums in one chunk of 20 in-edges (one memory latency per tile; 5 VGPRs
    # spilled) instead of two chunks of 10 (round 6: slower, tools/sessions/r6_05_wsu.sh)
    "wsu20": [("geot_node.hip", "constexpr int SEG_U_WS = 10;", "constexpr int SEG_U_WS = 20;", 1)],
    # the pair stream's blocks on the first N XCDs only (block b runs on XCD b mod 8; the others exit at
    # once): can a few XCDs' L2s and fabric links carry the store stream? (round-5 verdict item 4)
    **{f"pairxcd{n}": [("pair_tensor.hip", """  const int lane = threadIdx.x & 63;
  for (int k = job_begin; k < job_end; ++k) {
    if (!pq_wait(q + PQ_READY, (uint32_t)k + 1, patience)) {""", f"""  const int lane = threadIdx.x & 63;
  if ((int)(blockIdx.x & 7) >= {n}) return;
  for (int k = job_begin; k < job_end; ++k) {{
    if (!pq_wait(q + PQ_READY, (uint32_t)k + 1, patience)) {{""", 1)] for n in (1, 2, 3, 4, 6)},
    # the LDS-resident InitEdge capped at 160 VGPRs (three waves per SIMD + one pair-stream wave fit;
    # uncapped it allocates 168, so a CU hosting a pair-stream block cannot take its 12-wave block)
    "initres160": [("geot_init.hip", """__global__ __attribute__((amdgpu_flat_work_group_size(1, 64 * IRX_NW), amdgpu_waves_per_eu(IRX_NW / 4, IRX_NW / 4)))
void k_init_res_x32(InitArgs a, int ntiles) {""", """__global__ __attribute__((amdgpu_flat_work_group_size(1, 64 * IRX_NW), amdgpu_waves_per_eu(IRX_NW / 4, IRX_NW / 4),
                          amdgpu_num_vgpr(80)))
void k_init_res_x32(InitArgs a, int ntiles) {""", 1)],
    # the node kernels' LDS exchange rows at round 6's first padding (132 / 68 / 132 words: 2-way
    # conflicts left) instead of the conflict-free 136 / 66 / 130
    "ldspad4": [("geot_node.hip", """constexpr int LDS_ATTN = HID + 8;       // fp32 aggregated rows: 136 words
constexpr int LDS_N = HID + 4;          // bf16 n / h rows: 66 words
constexpr int LDS_T = 2 * HID + 4;      // bf16 FFN-hidden rows: 130 words""", """constexpr int LDS_ATTN = HID + 4;
constexpr int LDS_N = HID + 8;
constexpr int LDS_T = 2 * HID + 8;""", 1)],
    # the beside store window: four stores in flight per pair wave (three in the product)
    "inflight4": [("pair_tensor.hip", "constexpr int PAIR_INFLIGHT = 3;", "constexpr int PAIR_INFLIGHT = 4;", 1)],
    "inflight2": [("pair_tensor.hip", "constexpr int PAIR_INFLIGHT = 3;", "constexpr int PAIR_INFLIGHT = 2;", 1)],
    "inflight6": [("pair_tensor.hip", "constexpr int PAIR_INFLIGHT = 3;", "constexpr int PAIR_INFLIGHT = 6;", 1)],
    # round 6, static issue priority (MI355X_MICROARCH.md, two waves per SIMD, item 4): the edge ring's
    # second-dispatched half (waves 4-7) at s_setprio 1 for the whole launch / the first half instead
    "prio47": [("geot_edge.hip", "  st.fill();\n#pragma unroll 1\n", "  if (wave >= 4) __builtin_amdgcn_s_setprio(1);\n  st.fill();\n#pragma unroll 1\n", 1)],
    "prio03": [("geot_edge.hip", "  st.fill();\n#pragma unroll 1\n", "  if (wave < 4) __builtin_amdgcn_s_setprio(1);\n  st.fill();\n#pragma unroll 1\n", 1)],
    # the edge ring's waves 4-7 start ~512 cycles late (a stagger against lockstep SIMD partners, item 9)
    "stag": [("geot_edge.hip", "  st.fill();\n#pragma unroll 1\n", "  st.fill();\n  if (wave >= 4) __builtin_amdgcn_s_sleep(8);\n#pragma unroll 1\n", 1)],
    # k_node_ws's waves 4-7 at s_setprio 1
    "nodeprio": [("geot_node.hip", "  if constexpr (!FINAL) dma_blocks<NWS_NW>(s_q, W + NL_Q * BLK, 3 * MAT128);\n  // this wave's",
                  "  if (w >= 4) __builtin_amdgcn_s_setprio(1);\n  if constexpr (!FINAL) dma_blocks<NWS_NW>(s_q, W + NL_Q * BLK, 3 * MAT128);\n  // this wave's", 1)],
    # the pair stream's waves at s_setprio 2: their store instructions win issue over the GeoT waves
    # sharing their SIMD
    "pairprio": [("pair_tensor.hip", """  const int lane = threadIdx.x & 63;
  for (int k = job_begin; k < job_end; ++k) {
    if (!pq_wait(q + PQ_READY, (uint32_t)k + 1, patience)) {""", """  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_s_setprio(2);
  for (int k = job_begin; k < job_end; ++k) {
    if (!pq_wait(q + PQ_READY, (uint32_t)k + 1, patience)) {""", 1)],
    # InitEdge's positional rows read at half their bytes (features 0..63 twice: the traffic a bf16
    # copy of the fp32 tables would gather; timing only)
    "posh": [("geot_init.hip", """      const int f = 32 * b + 8 * q + 4 * h;
      set_quad(acc.v[b], q, ld4(rs + f) + ld4(rd + f));""", """      const int f = 32 * (b & 1) + 8 * q + 4 * h;
      set_quad(acc.v[b], q, ld4(rs + f) + ld4(rd + f));""", 1)],
    # CU-level spatial split of the two dedicated streams (environment-driven, diagnostic only):
    # DI_DIAG_GMASK=m takes m CUs per XCD away from the GeoT stream (and sizes its persistent grids to
    # the CUs left), DI_DIAG_PMASK=m puts the pair stream on exactly those m CUs per XCD (0: all CUs).
    # The set is balanced per XCD whether mask bit c maps to XCD c % 8 or to XCD c / 32: bit
    # c = 32 x + 8 j + y is in it iff (y - x) mod 8 < m / 4.
    "cusplit": [("streams.hip", """  std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
  for (int c = 0; c < cus; ++c) mask[(size_t)c >> 5] |= 1u << (c & 31);""", """  static int calls = 0;
  const int which = calls++ & 1;  // 0: the GeoT stream, 1: the pair stream (schedule_streams order)
  const char* ev = getenv(which ? "DI_DIAG_PMASK" : "DI_DIAG_GMASK");
  const int m = ev ? atoi(ev) : 0;
  std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
  for (int c = 0; c < cus; ++c) {
    const bool in = m > 0 && ((((c & 7) - (c >> 5)) & 7) < m / 4);
    if (which ? (m == 0 || in) : !in) mask[(size_t)c >> 5] |= 1u << (c & 31);
  }""", 1),
                ("geot.h", "  const int cus = device_cus();",
                 '  const int cus = device_cus() - 8 * (getenv("DI_DIAG_GMASK") ? atoi(getenv("DI_DIAG_GMASK")) : 0);', 1)],
    # the edge ring's three re-reads of the edge's own F row (res_connect, final_linear, O_edge) from
    # rows 0..31 instead (always L2-hot): the most keeping F on chip could buy (timing only). The z0
    # layer 0 re-reads nothing (it rebuilds F0's blocks) and is unchanged
    "reread0": [("geot_edge.hip", "  const u16* f_row = reinterpret_cast<const u16*>(a.f_in) + (int64_t)e * HID;\n  const u16* qkv",
                 "  const u16* f_row = reinterpret_cast<const u16*>(a.f_in) + (int64_t)e * HID;\n"
                 "  const u16* f_row0 = reinterpret_cast<const u16*>(a.f_in) + (int64_t)(e & 31) * HID;\n  const u16* qkv", 1),
                ("geot_edge.hip", "  if constexpr (!Z0) fr.load(f_row, h);\n  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // res_connect_linear",
                 "  if constexpr (!Z0) fr.load(f_row0, h);\n  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // res_connect_linear", 1),
                ("geot_edge.hip", "  if constexpr (!Z0) fr.load(f_row, h);\n  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // final_linear",
                 "  if constexpr (!Z0) fr.load(f_row0, h);\n  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // final_linear", 1),
                ("geot_edge.hip", "    if constexpr (!Z0) fr.load(f_row, h);                    // O_edge: re-read",
                 "    if constexpr (!Z0) fr.load(f_row0, h);                   // O_edge: re-read", 1)],
    # the edge ring's weight stages DMA'd at half their blocks (the slot's second half keeps stale
    # weights; timing only): how much of the edge layers' cost to the pair stream is their L2 -> LDS
    # weight stream (~16 TB/s of L2 reads chip-wide while the ring runs)
    "whalf": [("geot_edge.hip", "    const int off = EL_ORDER[si], n = EL_SIZE[si];  // the stage's run: first block, block count",
               "    const int off = EL_ORDER[si], n = EL_SIZE[si] / 2;", 1)],
    # the edge ring's weight stages all DMA'd from the blob's first blocks (same bytes, a 36-KiB
    # footprint that always hits L2; timing only): separates the stream's L2 misses from its bytes
    "ringw0": [("geot_edge.hip", "    const int off = EL_ORDER[si], n = EL_SIZE[si];  // the stage's run: first block, block count",
                "    const int off = 0, n = EL_SIZE[si];", 1)],
    # the edge ring's blocks of one XCD kept in step: after each tile (but a block's last ones), wave 0
    # adds to its XCD's counter and waits (<= 20 us) until every block of the XCD has finished that
    # tile, so the 32 blocks stay within one tile of each other and fewer of the layer's weight stages
    # are live in the XCD's L2 at once (the stream's L2 misses). Results
    # unchanged (A/B variant, correct outputs)
    "xcdbar": [("geot.h", """  const void* init_wmat = nullptr;
};

struct NodeArgs {""", """  const void* init_wmat = nullptr;
  uint32_t* xbar = nullptr;  // diag xcdbar: per-XCD tile counters (16 words apart)
};

struct NodeArgs {""", 1),
               ("geot_edge.hip", """    edge_x32_tile<MODE, GC, Z0>(a, st, e, valid, lane, h, wc2);
  }
}""", """    edge_x32_tile<MODE, GC, Z0>(a, st, e, valid, lane, h, wc2);
    const int G = (int)gridDim.x, x = (int)(blockIdx.x & 7);
    if (a.xbar && wave == 0 && (G & 7) == 0 && i + 1 < ntiles / G) {
      uint32_t* c = a.xbar + 16 * x;
      const uint32_t need = (uint32_t)((i + 1) * (G / 8));
      if (lane == 0) __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need &&
             __builtin_amdgcn_s_memrealtime() - t0 < 2000)
        __builtin_amdgcn_s_sleep(2);
    }
  }
}""", 1),
               ("geot_edge.hip", """  const PersistentGrid p = persistent_grid(a.Et, EdgeRingGeo::ROWS);
  hipLaunchKernelGGL((k_edge_x32_ring<MODE, GC, Z0>),""",
                """  const PersistentGrid p = persistent_grid(a.Et, EdgeRingGeo::ROWS);
  static uint32_t* xbar = nullptr;
  if (!xbar && hipMalloc(&xbar, 8 * 16 * sizeof(uint32_t)) != hipSuccess) xbar = nullptr;
  if (xbar && hipMemsetAsync(xbar, 0, 8 * 16 * sizeof(uint32_t), s) == hipSuccess) a.xbar = xbar;
  hipLaunchKernelGGL((k_edge_x32_ring<MODE, GC, Z0>),""", 1)],
}
# combinations (every substitution of each part)
DIAGS["prio47node"] = DIAGS["prio47"] + DIAGS["nodeprio"]
DIAGS["prio47pair"] = DIAGS["prio47"] + DIAGS["pairprio"]


def build_diag(name):
    tmp = tempfile.mkdtemp(prefix=f"di_diag_{name}_")
    try:
        src = os.path.join(tmp, "deepinteract_amd", "csrc")
        shutil.copytree(build.CSRC, src)
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tmp, "include"))
        for fname, old, new, count in DIAGS[name]:
            p = os.path.join(src, fname)
            text = open(p).read()
            if text.count(old) != count:
                raise SystemExit(f"diag {name}: pattern found {text.count(old)}x in {fname}, expected {count}")
            open(p, "w").write(text.replace(old, new))
        out = os.path.join(build.LIBDIR, "variants", f"diag_{name}", "libdeepinteract_amd.so")
        saved = build.CSRC, build.CFLAGS
        build.CSRC = src
        build.CFLAGS = [f for f in build.CFLAGS if not f.startswith("-I")] + [f"-I{os.path.join(tmp, 'include')}"]
        try:
            return build.build(force=True, defines=[f"DI_TIMING_DIAG_{name.upper()}=1"], out=out)
        finally:
            build.CSRC, build.CFLAGS = saved
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    for n in sys.argv[1:] or list(DIAGS):
        print(build_diag(n))
