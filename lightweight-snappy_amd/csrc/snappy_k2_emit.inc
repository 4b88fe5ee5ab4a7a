// snappy_k2_emit.inc -- the body of K2 (tokens -> Snappy bytes), included by its
// two entry points in snappy_kernels.hip: k2_emit_units (K2_RECORDS 0: unit u at
// u * unit, its tokens at u * tok_cap, its segment records at u * segs) and
// kr2_emit_records (K2_RECORDS 1: the record's places in `rec`, a K2Record; `in`
// and `n` are the record's own start and length).  Text, not a function template:
// moved into a function and inlined back, the same statements gave k2_emit_units
// other instructions (2,540 against 2,635, another register allocation), and the
// fixed-layout kernels keep theirs (tools/isa_identity.py).
// Names it expects: in, n, unit, hdr_mode, header_value, tokens, tok_cap, ntok,
// seg_off, segs, offsets, out (K2_RECORDS 1: in, n, hdr_mode, header_value, ntok,
// offsets, out, rec).
    __shared__ __attribute__((aligned(16))) uint8_t stage_[kK2Stage + 4 + 4 * 64 + 16];  // + alignment, per-lane dummies
    auto *const stage = (__attribute__((address_space(3))) uint8_t *)stage_;
    const uint32_t lane = threadIdx.x;
    const uint32_t u = blockIdx.x;
    const uint32_t nt = ntok[u];
#if K2_RECORDS
    const uint64_t base = 0;
    const uint32_t L = rec.L;
#else
    const uint64_t base = (uint64_t)u * unit;
    const uint32_t L = (uint32_t)((n - base) < unit ? (n - base) : unit);
#endif
    const uint8_t *src = in + base;
    uint8_t *dst = out + offsets[u];
    // 4-byte tokens (K1r: offset | (length - 4) << 16 | gap << 24, escapes in tok_full)
#if K2_RECORDS
    const uint32_t *tok = rec.tok, *tok_full = rec.tok_full;
#else
    const uint32_t *tok = reinterpret_cast<const uint32_t *>(tokens) + (uint64_t)u * tok_cap;
    const uint32_t *tok_full = reinterpret_cast<const uint32_t *>(tokens) + ((uint64_t)gridDim.x + u) * tok_cap;
#endif
    if (blockIdx.y == 0) {
        if (hdr_mode == SNAPPY_HDR_EVERY_UNIT) varint_put(L, dst, lane);
        // (K2_RECORDS: the entry point says which units are first ones -- block 0 of a long record)
        else if (hdr_mode == SNAPPY_HDR_FIRST_UNIT && (K2_RECORDS || u == 0)) varint_put(header_value, dst, lane);
    }
    // the next pass's token words (and the next segment's record) are loaded one
    // pass ahead, so their round trip overlaps this pass's literal loads
    uint32_t kwn[kK2Per];
    auto load_kw = [&](uint32_t c, uint32_t *k) {
#pragma unroll
        for (uint32_t i = 0; i < kK2Per; i++) {
            const uint32_t t = c + kK2Per * lane + i;
            k[i] = tok[t < nt ? t : 0u];
        }
    };
    auto load_se = [&](uint32_t sg) {
#if K2_RECORDS
        return *reinterpret_cast<const uint2 *>(rec.segu + 2 * (sg * kK2Seg <= nt ? sg : 0u));
#else
        return *reinterpret_cast<const uint2 *>(seg_off + 2 * ((uint64_t)u * segs + (sg * kK2Seg <= nt ? sg : 0u)));
#endif
    };
    if (blockIdx.y * kK2Seg <= nt) load_kw(blockIdx.y * kK2Seg, kwn);
    uint2 sen = load_se(blockIdx.y);
    for (uint32_t sg = blockIdx.y; sg * kK2Seg <= nt; sg += gridDim.y) {
    // K1r's table: the segment's output offset and the input position where
    // its first literal starts (the end of the previous segment's last token)
    const uint2 se = sen;
    sen = load_se(sg + gridDim.y);
    uint32_t o = se.x, carry = se.y;
    for (uint32_t c = sg * kK2Seg; c < (sg + 1) * kK2Seg && c <= nt; c += kK2Pass) {

    uint32_t gap[kK2Per], len[kK2Per], off[kK2Per], pe[kK2Per], litn[kK2Per], hl[kK2Per], sz[kK2Per];
    bool live[kK2Per];
    uint32_t lspan = 0;  // input bytes covered by the lane's tokens (literal + copy)
    // the lane's token words in one round trip (a lane past the end re-reads word 0:
    // no branch, so no load waits for the one before it), then the rare escapes
    uint32_t kw[kK2Per];
#pragma unroll
    for (uint32_t i = 0; i < kK2Per; i++) kw[i] = kwn[i];
    {
        uint32_t cn = c + kK2Pass;
        if (!(cn < (sg + 1) * kK2Seg && cn <= nt)) cn = (sg + gridDim.y) * kK2Seg;
        if (cn <= nt) load_kw(cn, kwn);
    }
#pragma unroll
    for (uint32_t i = 0; i < kK2Per; i++) {
        const uint32_t t = c + kK2Per * lane + i;
        const bool has = t < nt;  // else the pseudo-token (the tail literal) or nothing
        live[i] = t <= nt;
        const uint32_t k = has ? kw[i] : 0xFFFFFFFFu;
        const uint32_t lc = (k >> 16) & 0xFF, gc = k >> 24;
        off[i] = has ? k & 0xFFFF : 0u;
        gap[i] = has ? gc : 0u;
        len[i] = has ? lc + 4 : 0u;
        if (has && (lc == 255 || gc == 255)) {
            const uint32_t f = tok_full[t];
            gap[i] = f & 0xFFFF;
            len[i] = f >> 16;
        }
        lspan += gap[i] + len[i];
    }
    uint32_t span_tot;
    uint32_t cur = carry + wave_excl_scan(lspan, lane, &span_tot);
    uint32_t lsum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kK2Per; i++) {
        const uint32_t t = c + kK2Per * lane + i;
        pe[i] = cur;  // where the token's literal starts
        litn[i] = t < nt ? gap[i] : (t == nt ? L - cur : 0u);
        cur += gap[i] + len[i];
        hl[i] = litn[i] ? (litn[i] <= 60 ? 1 : (litn[i] <= 256 ? 2 : 3)) : 0;
        sz[i] = hl[i] + litn[i] + ((live[i] && len[i]) ? copy_bytes(len[i], off[i]) : 0);
        lsum += sz[i];
    }
    uint32_t total;
    uint32_t rel = wave_excl_scan(lsum, lane, &total);
    const bool staged = total <= kK2Stage;
    // the stage is laid out at the destination's alignment (stage byte sb + x is
    // output byte dst + o + x), so the copy-out below reads aligned LDS dwords
    const uint32_t sb = staged ? (uint32_t)(reinterpret_cast<uintptr_t>(dst + o) & 3) : 0u;
    uint64_t longs[kK2Per];
    uint32_t d0v[kK2Per];
    // every short literal's source dwords in one round trip: lanes with none read
    // the unit's first token words (in bounds, ignored)
    uint32_t lw[kK2Per][5], lsh[kK2Per];
    bool wide[kK2Per];
#pragma unroll
    for (uint32_t i = 0; i < kK2Per; i++) {
        wide[i] = base + pe[i] + 20 <= n;  // the aligned 20-byte read ends inside in[0, n)
        const bool ld = !SNAPPY_K2_NOLIT && staged && wide[i] && live[i] && litn[i] != 0 && litn[i] <= 16;
        const uintptr_t sa = reinterpret_cast<uintptr_t>(src + pe[i]);
        lsh[i] = (uint32_t)(sa & 3);
        const auto *aw = reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(
            ld ? sa - lsh[i] : reinterpret_cast<uintptr_t>(tok));
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) lw[i][j] = aw[j];
    }
#pragma unroll
    for (uint32_t i = 0; i < kK2Per; i++) {
        const bool wide_ok = wide[i];
        if (staged) put_element_lds(stage, rel + sb, src, pe[i], litn[i], hl[i], len[i], off[i], wide_ok, live[i], lane,
                                    lw[i], lsh[i]);
        else if (live[i]) put_element(dst + o + rel, src, pe[i], litn[i], hl[i], len[i], off[i], wide_ok);
        longs[i] = __ballot(live[i] && litn[i] > 16);
        d0v[i] = rel + sb + hl[i];
        rel += sz[i];
    }
#pragma unroll
    for (uint32_t i = 0; i < kK2Per && !SNAPPY_K2_NOLIT; i++) {
        if (staged) k2_long_literals(stage, src, longs[i], litn[i], pe[i], d0v[i], lane);
        else k2_long_literals(dst + o, src, in + n, longs[i], litn[i], pe[i], d0v[i], lane);
    }
    if (staged) {
        __builtin_amdgcn_wave_barrier();
        // stage[sb, sb + total) -> dst + o: byte head to a dword boundary, aligned
        // dwords (aligned in LDS too: sb + head is a multiple of 4), byte tail
        uint8_t *g = dst + o;
        uint32_t head = (4 - sb) & 3;
        if (head > total) head = total;
        if (lane < head) g[lane] = stage[sb + lane];
        const uint32_t nw = (total - head) >> 2;
        uint32_t *gw = reinterpret_cast<uint32_t *>(g + head);
        const auto *sw = reinterpret_cast<const __attribute__((address_space(3))) uint32_t *>(stage + sb + head);
        for (uint32_t k = lane; k < nw; k += 64) gw[k] = sw[k];
        const uint32_t tail0 = head + 4 * nw;
        if (lane < total - tail0) g[tail0 + lane] = stage[sb + tail0 + lane];
    }
    __builtin_amdgcn_wave_barrier();  // the stage is reused by the next pass
    o += total;
    carry += span_tot;
    }
    }
