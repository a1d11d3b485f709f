// pg_search_kernel_body.h -- the body of pg_search_kernel<NB, NS, Id, mode, DEF> and of pg_search_fixed_kernel<NB, NS, LEN>, included
// by pg_kernels.hip INSIDE the two kernels (NB, NS, Id, mode, DEF and LEN, search_read's fixed read length, are names of the
// including scope; the parameters are ref, prm, B).  Text, not a function: as a function inlined into the two kernels -- with
// parameters by reference or by value -- the body is optimised once on its own before it is inlined, and six of the existing
// kernels came out with other register allocations (<NB=3, NS=3, u32, BOTH, defaults>: 127 -> 131 SGPR spill slots, 24 -> 32 bytes
// of scratch; profiles/r08/README.md).  Included, every existing kernel compiles to what it was.
    // (a kernel of pg_rev_mismatch keeps the bit-reversed copies of the planes behind the two orientations: Lds::qp)
    constexpr int QPX = pg_rev_mismatch<NB, NS, Id, mode, DEF, false, LEN>() ? 4 : 2;
    __shared__ Lds<NB, Id, QPX> lds;
    const int lane = threadIdx.x;
    if (PG_WIN_DYN_BYTES(NB) != 0u) {
        // the window's dynamic tail must begin where the static LDS object ends (see Lds::win)
        extern __shared__ uint4 pg_dyn_lds[];
        if ((const char *)pg_dyn_lds != (const char *)&lds + sizeof(lds)) __builtin_trap();
    }
    if (PG_MM_IN_WIN(NB)) {
        for (int w = lane; w < 16 * NB + 16; w += WAVE) {
            u32 v = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) v |= (u32)max_mismatch_at(prm.mm_bp, 4 * w + k) << (8 * k);
            lds.win[w].w = v;
        }
    } else
        for (int L = lane; L < 64 * NB + 64; L += WAVE) lds.mm_tab[L] = (uint8_t)max_mismatch_at(prm.mm_bp, L);
    if (lane < PG_CHR_TAB_N(NB) && lane < ref.n_chr) {
        const u64 wo = ref.chr_word_off[lane];
        lds.chr_tab[lane] = make_uint2((u32)wo, (wo >> 32) == 0ull ? ref.chr_size[lane] : 0u);
    }
    PG_SYNC();
    Search S;
    S.queue = lds.queue;
    S.win = lds.win;
    S.bufA = lds.bufA;
    S.bufB = lds.bufB;
    S.hdrB = lds.hdrB;
    S.ringB = lds.ringB;
    S.accB = lds.accB;
    S.mm_tab = lds.mm_tab;
    S.chr_tab = lds.chr_tab;
    u64 *qplanes = lds.qp;                        // [0]: forward, [1]: reversed consumption order
    if (lane < 4 * QPX * NB) qplanes[lane] = 0ull;   // (blocks beyond the batch's plane layout are never written)
    // The open candidate pass (pg_open_pass) reads its queue slot in every lane: a slot no pass has written yet holds a valid
    // position from the start (not 0: a kind-B candidate at window position 0 would read below the window), and what a pass leaves
    // in it is one -- so an idle lane never forms an LDS address from data nobody wrote.
    if (pg_open_pass<NB, NS, Id, mode, DEF, false, LEN>() && lane < PG_PASS(NB)) lds.queue[lane] = PG_QUEUE_IDLE(NB);
#ifdef PG_TIMING
    S.t_acc = lds.t_acc;
    S.t_last = &lds.t_last;
    if (lane == 0) {
        for (int k = 0; k < 12; k++) S.t_acc[k] = 0u;
        *S.t_last = __builtin_readcyclecounter();
    }
    S.t_base = 1;
#endif

    // Reads claimed per atomic (PgDevBatch::claim, worked out by pg_launch_search): a workgroup's share of the launch in the fewest
    // equal claims of at most PG_CLAIM reads.  The host
    // launches one workgroup per PG_CLAIM reads up to the chip's resident slots, so up to 57 k reads every wave takes exactly one claim
    // of eight; between that and a few hundred thousand reads the share is 8..64 reads and claims of exactly eight would leave some
    // waves a whole claim more than others (100 000 reads: 14 per wave = two claims of seven).  Measured, seven waves per SIMD:
    // 50 000 reads 0.262 ms with claims of two, 0.23 with eight; 100 000: 0.403 -> 0.36; 5000 reads on 633 workgroups 0.106 either way,
    // and 0.125 on 5008 workgroups of one read each -- a small launch pays for the NUMBER of workgroups.  A wave that looks at the
    // other parts' counters before claiming from them (the walk over the eight parts at the end of a launch is one atomic per wave
    // and address) gained nothing.
    // (Claims of ONE read for the last round and a half of a launch, to shorten its tail, were measured and rejected: a claim
    // is a dependent chain atomic -> records -> first window, 2 us that eight reads share -- 262 144 reads 0.94 -> 0.98 ms.)
    // Nothing but `part` and `tried` lives from one claim to the next: the launch's size comes from the kernarg segment again.
    // (Quarter claims for the last rounds of a launch that packs in place -- the waves finish spread over one claim's duration -- were
    // measured and rejected, round 6: a claim is a dependent chain atomic -> pack (three HBM round trips) -> records, and the short
    // claims cost more than the shorter tail gives back: 2 M reads at -x 5 22.16 -> 22.24 ms, 2 M at -x 2 4.55 -> 4.58 / 4.70 ms
    // for two / four rounds.  Claims of eight, as without the pack: sixteen and more lose at -x 5, where a read takes 79 us.)
    uint32_t part = blockIdx.x % PG_N_XCD, tried = 0;
    while (tried < PG_N_XCD) {
        const uint32_t n = KA(B, n_reads);
        const uint32_t claim = KA(B, claim);              // (pg_launch_search: the share of a workgroup in the fewest equal claims <= PG_CLAIM)
        const uint32_t per = n / PG_N_XCD;
        const uint32_t lo = part * per, hi = part + 1 == PG_N_XCD ? n : lo + per;
        // (the single-lane atomics by hand: the compiler wraps an atomicAdd in its wave-reduction form -- exec juggling, mbcnt,
        // bcnt, a multiply -- some 25 instructions each)
        uint32_t got = 0;
        uint32_t *ctr = KA(B, work_ctr) + part * 16u;
        if (lane == 0) asm volatile("global_atomic_add %0, %1, %2, %3 sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(got) : "v"(0u), "v"(claim), "s"(ctr) : "memory");
        got = (u32)uni((int)got);
        if (got >= hi - lo) {                             // this part is exhausted
            part = part + 1 == PG_N_XCD ? 0 : part + 1;
            tried++;
            continue;
        }
        const uint32_t first = lo + got, end = hi - first < claim ? hi : first + claim;
        PG_T(S, 11);
        uint32_t no_touch = ~0u;                          // the read that must not touch its successor's record (none)
        {
            // PACK IN PLACE (PgDevBatch::soa set; any mode -- the two seams' launches pack their reads too): the wave builds the records and bit planes of its claim from the SoA arrays
            // before it searches them -- the pack kernel's body on the claim's reads.  A streaming transpose (HBM-bound on its own,
            // 3 TB/s) inside a kernel that is bound by instruction issue and leaves 90 % of the HBM bandwidth idle: ~30 instructions
            // per read instead of a launch of its own in front of this one.  What the wave wrote it reads back itself, through the
            // caches of its own CU and XCD (scalar loads of the records, vector loads of the planes): the stores' completion is all
            // there is to wait for.  (The host sets soa only when the batch's plane layout is this kernel's: plane_blocks == NB.)
            const PgSoaIn *soa = KA(B, soa);
            if (soa) {
                const PgSoaIn a = *soa;
                pack_block<NB>(a, const_cast<PgInRec *>(KA(B, in)), KA(B, first_read) + first, 0u, end - first, (u32)lane_now());
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                // (a read touches the next read's record while it waits for its first window: the claim's last read would bring
                // the line of a record nobody has written yet into the scalar cache, where its owner might then find it)
                no_touch = end - 1u;
            }
        }
        // run-pool slots of the claim's reads: one atomic per claim
        u32 res = 0u;
        {
            const u32 shard = blockIdx.x & (PG_POOL_SHARDS - 1u);
            uint32_t *cur = KA(B, pool_used) + shard * 16u;
            if (lane == 0) asm volatile("global_atomic_add %0, %1, %2, %3 sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(res) : "v"(0u), "v"(claim * PG_RESERVE), "s"(cur) : "memory");
            res = (u32)uni((int)res);
            const u32 res_fits = (u64)res + (u64)(claim * PG_RESERVE) <= (u64)KA(B, pool_shard_cap) ? 1u : 0u;
            res += shard * KA(B, pool_shard_cap);
            for (uint32_t i = first; i < end; i++)
                search_read<NB, NS, Id, mode, DEF, false, LEN>(ref, prm, B, S, qplanes, KA(B, first_read) + i, i != no_touch ? 1 : 0, lane_now(),
                                          res + (i - first) * PG_RESERVE, res_fits);
            PG_T(S, 10);
        }
    }
#ifdef PG_TIMING
    if (lane == 0) {
        u64 *dg = (u64 *)(KA(B, work_ctr) + PG_WORK_CTRS * 16u);
        for (int k = 0; k < 12; k++) atomicAdd((unsigned long long *)(dg + k), (unsigned long long)S.t_acc[k]);
    }
#endif
