// pg_report.hip -- the fifth part of the device classifier: what a report writer takes from the candidate lists and
// the points, gathered per table member and per read, so that neither has to leave the GPU.  The host statement of the same function
// is pg_host_report.hpp; the two must agree byte for byte.
//   pg_report_summary_kernel  one thread per read: close end, far end, rc_flag, UP_Close.back() and UP_Far[0] from the run lists.
//   pg_report_read_kernel     one thread per member of the seven member lists: the pair its read's pg_event_read names, the carried
//                             NT_size, for table 1 the LengthStr NT_str is cut behind (point_at over the run list), for table 2 the
//                             DI companion.  A gather: a few dozen bytes per member, nothing wave-wide.
//   pg_report_cut_kernel      pg_device_batch_classify's max_listed: one thread per read over its seven count bytes.
// Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(sizeof(pg_report_read) == 48 && sizeof(pg_report_summary) == 12 && sizeof(pg_variant_cand) == 32, "layouts of the records");
static_assert(offsetof(pg_variant_cand, nt_rot) == 20 && offsetof(pg_variant_cand, bp) == 24 && offsetof(pg_variant_cand, close_idx) == 26 &&
                  offsetof(pg_variant_cand, far_idx) == 28 && offsetof(pg_report_read, cand) == 4 && offsetof(pg_report_read, nt_size) == 36 &&
                  offsetof(pg_report_read, table) == 38 && offsetof(pg_report_read, flags) == 39 && offsetof(pg_report_read, bp0) == 40 &&
                  offsetof(pg_report_read, di_bp) == 42 && offsetof(pg_report_read, di_nt_rot) == 44,
              "the dwords the record kernel reads and writes");

extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_report_summary_kernel(PgReportArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const PgOutRec o = a.out[i];
    pg_report_summary s;
    s.close_abs = 0u;
    s.close_len = 0;
    s.far_chr = 0;
    s.flags = 0;
    s.rc_flag = o.rc_flag;
    s.reserved = 0;
    // (a list that does not lie in the pool counts as empty: nothing is read beyond it)
    if (o.close_cnt && (unsigned long long)o.close_off + o.close_cnt <= a.pool_runs) {
        const pg_run r = a.pool[o.close_off + o.close_cnt - 1u];     // UP_Close.back(): the last point of the last run
        const u32 d = (u32)r.len_last - r.len_first;
        s.close_abs = (r.flags & PG_RUN_BACKWARD) ? r.abs_loc_first - d : r.abs_loc_first + d;
        s.close_len = (int16_t)r.len_last;
        s.flags |= PG_RS_CLOSE;
    }
    if (o.far_cnt && (unsigned long long)o.far_off + o.far_cnt <= a.pool_runs) {
        const pg_run r = a.pool[o.far_off];                          // UP_Far[0]: the first point of the first run
        s.far_chr = r.chr_id;
        s.flags |= PG_RS_FAR;
        if (r.flags & PG_RUN_ANTISENSE) s.flags |= PG_RS_FAR_ANTISENSE;
        if (s.flags & PG_RS_CLOSE) {
            const uint32_t c0 = a.pool[o.close_off].abs_loc_first;   // UP_Close[0] against UP_Far[0]
            if (c0 < r.abs_loc_first) s.flags |= PG_RS_CLOSE_LEFT;
            if (c0 > r.abs_loc_first) s.flags |= PG_RS_CLOSE_RIGHT;
        }
    }
    a.summaries[i] = s;
}

extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_report_read_kernel(PgReportArgs a)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= a.start[PG_REPORT_TABLES]) return;
    u32 t = 0;
    for (u32 k = 1; k < PG_REPORT_TABLES; k++) t += (u32)(m >= a.start[k]);
    const u32 word = t < PG_EVENT_TABLES ? a.ev_members[m] : a.sv_members[m - a.start[PG_EVENT_TABLES]];
    const u32 read = t < PG_EVENT_TABLES ? word : word & ~PG_SVEV_MEMBER_DUP;
    // The record as its twelve dwords, the pair as its eight (pg_variant_cand: bp | close_idx << 16 in dword 6, far_idx in the low
    // half of dword 7, nt_rot dword 5): every field in a register of its own, no private copy of a struct.
    u32 cw[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    u32 r_read = 0, r_nt = 0, r_table = 0, r_flags = 0;
    int32_t r_bp0 = 0, r_di_bp = 0, r_di_rot = 0;
    if (read < a.n) {
        const pg_event_read er = a.reads[read];
        const u32 kind = er.kind, slot = er.slot;
        const pg_variant_cand *c = nullptr;
        if (kind < 2u) {
            if (slot < PG_VARIANT_CANDS) c = a.cands + ((size_t)read * 2u + kind) * PG_VARIANT_CANDS + slot;
        } else if (kind <= (u32)PG_SV_INV_NT) {
            const u32 slot0 = kind == PG_SV_DI ? 0u : kind == PG_SV_TD ? 1u : kind == PG_SV_TD_NT ? 1u + PG_VARIANT_CANDS
                            : kind == PG_SV_INV ? 2u + PG_VARIANT_CANDS : 2u + 2u * PG_VARIANT_CANDS;
            const u32 cap = (kind == PG_SV_TD || kind == PG_SV_INV) ? PG_VARIANT_CANDS : 1u;
            if (slot < cap) c = a.sv_cands + (size_t)read * PG_SV_SLOTS + slot0 + slot;
        }
        if (c) {
            r_read = read;
            const u32 *cp = (const u32 *)c;
#pragma unroll
            for (int k = 0; k < 8; k++) cw[k] = cp[k];
            r_nt = er.nt_size;
            r_table = t;
            if (t >= PG_EVENT_TABLES && (word & PG_SVEV_MEMBER_DUP)) r_flags |= PG_RR_DUP;
            if (t == 1u) {
                // what variant_pair_from_cand cuts NT_str behind: the close point for a '+' anchor, the far point otherwise
                const PgOutRec o = a.out[read];
                const bool plus = a.strand[read] == '+';
                int32_t len0 = 0;
                // (a list that does not lie in the pool counts as empty, like an index beyond its list: LengthStr 0)
                if (plus) {
                    if ((unsigned long long)o.close_off + o.close_cnt <= a.pool_runs) len0 = point_at(a.pool + o.close_off, o.close_cnt, cw[6] >> 16).len;
                } else if ((unsigned long long)o.far_off + o.far_cnt <= a.pool_runs) {
                    len0 = point_at(a.pool + o.far_off, o.far_cnt, cw[7] & 0xffffu).len;
                }
                r_bp0 = (int32_t)(int16_t)(len0 - 1);
            }
            if (t == 2u && (a.sv_counts[(size_t)read * PG_SV_KINDS] & ~PG_VARIANT_MORE) >= 1u) {
                const u32 *di = (const u32 *)(a.sv_cands + (size_t)read * PG_SV_SLOTS);
                r_flags |= PG_RR_DI;
                r_di_bp = (int32_t)(di[6] & 0xffffu);
                r_di_rot = (int32_t)di[5];
            }
        }
    }
    u32 *dst = (u32 *)(a.records + m);
    dst[0] = r_read;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[1 + k] = cw[k];
    dst[9] = r_nt | (r_table << 16) | (r_flags << 24);          // nt_size, table, flags
    dst[10] = ((u32)r_bp0 & 0xffffu) | ((u32)r_di_bp << 16);    // bp0, di_bp
    dst[11] = (u32)r_di_rot;
}

extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_report_cut_kernel(uint8_t *counts, uint8_t *sv_counts, u32 n, u32 max_listed)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= n) return;
    for (u32 k = 0; k < 2u + PG_SV_KINDS; k++) {
        uint8_t *p = k < 2u ? counts + (size_t)i * 2u + k : sv_counts + (size_t)i * PG_SV_KINDS + (k - 2u);
        const u32 c = *p;
        if ((c & ~PG_VARIANT_MORE) > max_listed) *p = (uint8_t)(max_listed | PG_VARIANT_MORE);
    }
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
int pg_report_launch(const PgReportArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (a->n) hipLaunchKernelGGL(pg_report_summary_kernel, dim3((a->n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK), dim3(PG_EV_BLOCK), 0, st, *a);
    const u32 nm = a->start[PG_REPORT_TABLES];
    if (nm) hipLaunchKernelGGL(pg_report_read_kernel, dim3((nm + PG_EV_BLOCK - 1u) / PG_EV_BLOCK), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_report_cut_launch(uint8_t *counts, uint8_t *sv_counts, uint32_t n, uint32_t max_listed, void *stream)
{
    if (!n) return 0;
    hipLaunchKernelGGL(pg_report_cut_kernel, dim3((n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK), dim3(PG_EV_BLOCK), 0, (hipStream_t)stream, counts, sv_counts, n,
                       max_listed);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
