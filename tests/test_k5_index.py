"""The block index of a foreign SINGLE stream -- K5p (k5a_chunk_walk, k5b1_compose,
k5b_carry, k5b3_fill, k5c_mark, k5d_result) and the one-wave k5_index_stream -- on
planted streams: every seam of the chunk-parallel walk reached on purpose.

Streams are built element by element (golden_inputs.enc_literal / enc_copy / varint)
over fresh random bytes, at absolute stream positions: the 16,384-byte chunks start
at the end of the preamble, so a builder is given the preamble's length and checks it
at the end.

* k5_serial(stream, max_units) restates k5_index_stream (HEADER, CAPACITY, TRUNCATED,
  UNSUPPORTED, OVERRUN in its order) and is the expected value of every case; for
  valid streams the entries are recomputed from the element list the stream was
  built from and must agree.
* k5p_model(stream) restates K5p's control flow with the kernel's integer widths:
  K5a's checkpoint loop, the switch to one chain, the error exit and X / O / P;
  K5b1's composition; k5b_carry's fast, prefetch and demand blocks, the demand skip,
  step's lookup and walk, parse_la's lookahead; K5b3's fill; K5c's batches (the lane
  model of tools/k5_model.py, with its window).  Every loop has an iteration cap: a
  walk that stops advancing raises Stall on the CPU.  With parent=True it runs the
  arithmetic of the build before the fix (no early return in K5a, the error exit
  clen + 1 - c0): on a stream with clen = m * 16384 + h.len - 1 (h.len >= 2) the last
  chunk starts at clen + 1, end_rel wraps to 0xFFFFFFFF, every lane's error exit is 0
  and walk_to never ends -- the model trips its cap there, and not with the fix.
* test_inputs_have_their_properties (no GPU) runs the model over every input, checks
  Ent / Base / offsets against the serial walk and asserts that each edge of EDGES is
  reached, naming the inputs that reach it.

Two cases of the length list have no valid stream and are TRUNCATED ones instead: a
4-byte preamble needs N >= 2^21, and 65,536 bytes of 64-byte copies decode to less
than 1.4 MB, so the m = 4, h.len = 4 streams declare 2^21 and end early.

N = 0: the serial walk writes offsets[0] = h.len (the end of the chain); K5p wrote
nothing there and now does the same (k5c_mark, block 0).

One constant changed in a scratch build, GPU tests of this file that then fail: the
lookup limit (E - c0 < 65): [chunk_edges] and its three misaligned copies; skip >> 25:
test_index_large; a restage of half the window: 42 tests.  kDemand, SNAPPY_K5_WIN and
`<= N` on the fast path give the same index: which path ran shows in the
model's trace only.

GPU: for every input index_device with OPT_SERIAL_INDEX 0 and 1 gives k5_serial's
code, N and entries bit for bit (the entries past the index untouched); every valid
stream is decoded from that index (SINGLE) and equals the oracle's decode."""
import collections
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import snappy_amd
from golden_inputs import enc_copy, enc_literal, varint

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import k5_model  # noqa: E402

B = 65536
S, NBLK, CHECK, WIN, G, KDEMAND = 16384, 64, 192, 4096, 8, 8  # K5_S, chunks per block, kCheck, K5_WIN, K5_G, kDemand
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
ESC, ESC64, SKIP, BAD = M32, M64, M64, 1 << 62  # kK5Esc, kK5Esc64, K5_SKIP, kK5Bad
OK, HEADER, TRUNC, OVERRUN, CAPACITY, UNSUP = 0, -2, -3, -5, -6, -9
MAX_UNITS = (1 << 20) + 1  # Codec.index_tensor's


class Stall(Exception):
    """A modelled loop passed its iteration cap: the kernel would not end."""


# ---------------------------------------------------------------------------
# stream builder
# ---------------------------------------------------------------------------
class SB:
    """Elements appended at known absolute positions (preamble of hlen bytes)."""

    def __init__(self, hlen, seed):
        self.hlen, self.body, self.op, self.elems = hlen, bytearray(), 0, []
        self.rng = np.random.default_rng(seed)
        self.counted = True  # False: bytes after N

    @property
    def pos(self):
        return self.hlen + len(self.body)

    def _add(self, enc, ln):
        if self.counted:
            self.elems.append((self.pos, len(enc), ln))
            self.op += ln
        self.body += enc

    def lit(self, n, width=-1):
        self._add(enc_literal(self.rng.bytes(n), width), n)

    def lit_size(self, size):
        """A literal of `size` stream bytes (>= 2)."""
        if size <= 61:
            self.lit(size - 1, 0)
        elif size <= 258:
            self.lit(size - 2, 1)
        elif size <= 65539:
            self.lit(size - 3, 2)
        else:
            self.lit(size - 4, 3)

    def copy(self, ln, kind=2, off=None):
        if off is None:
            off = 1 + int(self.rng.integers(0, min(self.op, 2047 if kind == 1 else 60000)))
        self._add(enc_copy(ln, off, kind), ln)

    def filler(self, lo, hi, room):
        """One filler element: a literal of lo..hi stream bytes, or a copy-2."""
        if self.op > 0 and room >= hi + 5 and self.rng.integers(0, 4) == 0:
            self.copy(int(self.rng.integers(1, 65)))
        else:
            self.lit_size(int(self.rng.integers(lo, hi + 1)))

    def fill_to(self, target, lo=20, hi=61):
        """Filler elements until the next element starts exactly at `target`."""
        while self.pos < target:
            g = target - self.pos
            assert g >= 2, (self.pos, target)
            if g <= hi + 1:
                self.lit_size(g if g <= hi else g - 2)
            else:
                self.filler(lo, hi, g - 2)
        assert self.pos == target

    def fill_out(self, target_op, lo=20, hi=61):
        """Filler until the output is within 200 bytes below target_op."""
        while self.op < target_op - 200:
            self.filler(lo, hi, 1 << 30)

    def out_to(self, target_op):
        while self.op < target_op:
            self.lit(min(60, target_op - self.op))

    def sync(self, target_x, target_op, last="lit"):
        """Copies and one literal that end at stream position target_x with output target_op."""
        g, r = target_x - self.pos, target_op - self.op
        d = r - g + 3
        a = max(1, -(-d // 61), -(d // 2))
        n = g - 3 * a - 3
        t = r - n
        assert 1 <= n <= 65536 and a <= t <= 64 * a, (g, r, a, n, t)
        lens = [t // a + (1 if i < t % a else 0) for i in range(a)]
        if last == "lit":
            for ln in lens:
                self.copy(ln)
            self.lit(n, 2)
        else:
            self.lit(n, 2)
            for ln in lens:
                self.copy(ln)
        assert self.pos == target_x and self.op == target_op

    def raw(self, data):
        self.body += data

    def finish(self, n=None):
        pre = varint(self.op if n is None else n)
        if len(pre) != self.hlen:
            raise ValueError("preamble length")
        return pre + bytes(self.body)


def index_from_elems(elems, n):
    """The index of a valid stream from its element list (start, size, length)."""
    units = (n + B - 1) // B
    offs, op, end = {0: 0}, 0, elems[0][0] if elems else 0
    for x, size, ln in elems:
        if op >= n:
            break
        u = op // B + 1
        while u * B < op + ln and u * B < n:
            offs[u] = x | ((u * B - op) << 40)
            u += 1
        op += ln
        end = x + size
        if op % B == 0 and op < n:
            offs[op // B] = end
    assert op == n
    offs[units] = end
    return [offs[i] for i in range(units + 1)]


# ---------------------------------------------------------------------------
# k5_serial: k5_index_stream restated
# ---------------------------------------------------------------------------
def k5_serial(s, max_units=MAX_UNITS, chain=None):
    """(status, N, units, entries or None); chain, if a list, receives (start, output)
    of every element walked and of the end of the chain."""
    clen, n, ip, done = len(s), 0, 0, False
    for k in range(10):
        if ip >= clen:
            break
        byte = s[ip]
        ip += 1
        n |= ((byte & 0x7F) << (7 * k)) & M64
        if not byte & 0x80:
            done = True
            break
    st = OK if done else HEADER
    units = ((n + B - 1) & M64) // B
    if st == OK and units >= max_units:
        st = CAPACITY
    offs = {}
    if st == OK and units:
        offs[0] = 0
    op, unit = 0, 1
    while st == OK and op < n:
        if ip >= clen:
            st = TRUNC
            break
        x, tag = ip, s[ip]
        t = tag & 3
        if t == 0:
            ln = (tag >> 2) + 1
            ip += 1
            if ln > 60:
                kk = ln - 60
                if ip + kk > clen:
                    st = TRUNC
                    break
                ln = int.from_bytes(s[ip:ip + kk], "little") + 1
                ip += kk
            ip += ln
        elif t == 1:
            ln = ((tag >> 2) & 7) + 4
            ip += 2
        else:
            ln = (tag >> 2) + 1
            ip += 3 if t == 2 else 5
        if ip > clen:
            st = TRUNC
            break
        while unit * B < op + ln and unit * B < n:
            skip = unit * B - op
            if skip >> 24 or x >> 40:
                st = UNSUP
                break
            offs[unit] = x | (skip << 40)
            unit += 1
        if st != OK:
            break
        if chain is not None:
            chain.append((x, op))
        nb = unit * B
        op += ln
        if op == nb and op < n:
            offs[unit] = ip
            unit += 1
        if op > n:
            st = OVERRUN
            break
    if st == OK:
        offs[units] = ip
        if chain is not None:
            chain.append((ip, op))
    return st, n, units, ([offs[i] for i in range(units + 1)] if st == OK else None)


def true_chunks(s):
    """(Ent, Base) per chunk of a valid stream from the serial chain: the first element
    start at or past the chunk start if it lies in the chunk and before N, else SKIP."""
    chain = []
    st, n, _, _ = k5_serial(s, chain=chain)
    assert st == OK
    hlen = next(k for k in range(10) if not s[k] & 0x80) + 1
    clen, nch = len(s), (len(s) + S - 1) // S
    ent, base, i = [], [], 0
    for c in range(nch):
        c0 = hlen + c * S
        end = min(c0 + S, clen)
        while i < len(chain) - 1 and chain[i][0] < c0:
            i += 1
        x, op = chain[i] if chain else (hlen, 0)
        if x >= c0 and x < end and op < n:
            ent.append(x)
            base.append(op)
        else:
            ent.append(SKIP)
            base.append(None)
    return ent, base


# ---------------------------------------------------------------------------
# parse tables: the element at every stream position (k5_parse / k5_parse_img)
# ---------------------------------------------------------------------------
class Par:
    def __init__(self, s):
        self.s, self.clen = s, len(s)
        self.tab = None
        if self.clen <= 4 << 20:
            n = self.clen
            b = np.frombuffer(s + bytes(8), np.uint8).astype(np.int64)
            tag = b[:n]
            t, m = tag & 3, tag >> 2
            k = np.where((t == 0) & (m >= 60), m - 59, 0)
            v = b[1:n + 1] | (b[2:n + 2] << 8) | (b[3:n + 3] << 16) | (b[4:n + 4] << 24)
            lv = np.where(k == 0, m, v & ((1 << (8 * k)) - 1))
            ln = np.where(t == 0, lv + 1, np.where(t == 1, (m & 7) + 4, m + 1))
            hb = np.where(t == 0, 1 + k, np.array([0, 2, 3, 5])[t])
            size = np.where(t == 0, hb + ln, hb)
            self.tab = (hb.tolist(), size.tolist(), ln.tolist())

    def __call__(self, x):
        """(ok, size, len) as k5_parse_img over a zero-padded image; x >= clen: not ok."""
        if x >= self.clen:
            return False, 2, 1
        if self.tab:
            return x + self.tab[0][x] <= self.clen, self.tab[1][x], self.tab[2][x]
        return k5_model.parse(self.s, x)

    def kind(self, x):
        t = self.s[x] & 3
        if t:
            return "C%d" % (1, 2, 4)[t - 1]
        m = self.s[x] >> 2
        return "L%d" % (1 + (m - 59 if m >= 60 else 0))


# ---------------------------------------------------------------------------
# k5p_model
# ---------------------------------------------------------------------------
def k5p_model(s, parent=False, max_units=MAX_UNITS):
    """K5p restated.  Returns dict(status, n, units, offsets, ent, base, tr) with tr a
    Counter of the edges reached."""
    tr = collections.Counter()
    clen, par = len(s), Par(s)
    n, hlen, hst = 0, 0, HEADER
    for k in range(min(10, clen)):
        n |= ((s[k] & 0x7F) << (7 * k)) & M64
        if not s[k] & 0x80:
            hlen, hst = k + 1, OK
            break
    nch = (clen + S - 1) // S
    nblk = (nch + NBLK - 1) // NBLK
    units = ((n + B - 1) & M64) // B

    # ---- K5a ----
    def chain_nomark(c0, x, end_rel, bad):
        op, nb = 0, 0
        while x < end_rel:
            nb += 1
            if nb > S:
                raise Stall("k5_chain<false>")
            ins, l0 = [], 0
            while l0 < 64 and len(ins) < 32 and (x & M32) + l0 < end_rel:
                p = par(c0 + (x & M32) + l0)
                ins.append((l0, p))
                l0 += min(p[1], 64)
            x0, err = x, False
            for l, p in ins:  # the elements before the first bad header run
                if not p[0]:
                    err = True
                    break
                x0, op = x + l + p[1], op + p[2]
            x = bad if err else x0
        return x, op

    X, O, P = [None] * nch, [None] * nch, [None] * nch
    for c in range(nch):
        c0 = hlen + c * S
        if not parent and c0 >= clen:
            X[c], O[c], P[c] = [c0] * 64, [0] * 64, [ESC] * 64
            tr["k5a_start_at_or_past_clen"] += 1
            continue
        end_rel = (S if c0 + S < clen else (clen - c0) & M64) & M32
        bad = (clen + 1 - c0) & M64 if parent else BAD
        if end_rel < 64:
            tr["k5a_short_last_chunk"] += 1
        x, cum = list(range(64)), [0] * 64
        lim, ncp = CHECK, 0
        while True:
            ncp += 1
            if ncp > S // CHECK + 2:
                raise Stall("K5a checkpoints")
            lm = min(end_rel, lim)
            for l in range(64):
                xl, cl, it = x[l], cum[l], 0
                while xl < lm:
                    it += 1
                    if it > CHECK:
                        raise Stall("walk_to: chunk %d (c0 = %d, clen = %d) lane %d stands at %d"
                                    % (c, c0, clen, l, xl))
                    ok, size, ln = par(c0 + (xl & M32))
                    if not ok:
                        xl = bad
                    else:
                        cl += ln
                        xl += size
                x[l], cum[l] = xl, cl
            opn = [l for l in range(64) if x[l] < end_rel]
            if not opn:
                tr["k5a_never_merged" if ncp > 2 else "k5a_all_done_early"] += 1
                break
            x1 = x[opn[0]] & M32
            if all(x[l] & M32 == x1 for l in opn):
                xe, oe = chain_nomark(c0, x1, end_rel, bad)
                for l in opn:
                    x[l], cum[l] = xe, cum[l] + oe
                tr["k5a_merged_at_checkpoint_1" if ncp == 1 else "k5a_merged_at_checkpoint_2" if ncp == 2
                   else "k5a_merged_after_checkpoint_2"] += 1
                break
            lim += CHECK
        X[c] = [(c0 + v) & M64 for v in x]
        O[c] = cum
        row = []
        for l in range(64):
            nx = (x[l] - S) & M64
            good = c0 + 2 * S <= clen and x[l] >= S and nx < 64 and cum[l] < 1 << 24
            row.append((nx | (cum[l] << 8)) & M32 if good else ESC)
            if cum[l] >= 1 << 24:
                tr["esc_output_2^24"] += 1
            if end_rel == S and x[l] < BAD and S <= x[l]:
                if nx >= 64:
                    tr["esc_exit_past_byte_63"] += 1
                elif c0 + 2 * S > clen:
                    tr["esc_last_full_chunk"] += 1
        P[c] = row

    # ---- K5b1 ----
    F = []
    for b in range(nblk):
        row = []
        for e in range(64):
            cur, out, esc = e, 0, NBLK * b + NBLK > nch
            for j in range(NBLK):
                w = P[min(NBLK * b + j, nch - 1)][cur & 63]
                esc = esc or w == ESC
                out += w >> 8
                cur = w & 0xFF
            row.append(ESC64 if esc else cur | (out << 8))
        F.append(row)

    # ---- K5b2 (k5b_carry) ----
    ent, base_of = [None] * nch, [None] * nch
    BE, BB = [None] * nblk, [None] * nblk
    st8 = dict(E=hlen, base=0, lookups=0)
    la = dict(idx={}, ok=[False] * 64, size=[0] * 64, ln=[0] * 64, armed=False)

    def kparse(x):  # k5_parse: nothing at or past clen
        return par(x) if x < clen else None

    def parse_la(x):
        if x in la["idx"]:
            k = la["idx"][x]
            tr["la_hit"] += 1
            return la["ok"][k], la["size"][k], la["ln"][k]
        r = kparse(x)
        if r is None:
            return False, 0, 0
        ok, size, ln = r
        if ok and size >= 64:
            if la["armed"]:
                tr["la_miss_other_size"] += 1
            la["armed"], la["idx"] = True, {}
            for l in range(64):
                lx = (x + l * size) & M64
                la["idx"].setdefault(lx, l)
                q = kparse(lx)
                if q is None:
                    la["ok"][l] = False
                    tr["la_lane_past_clen"] += 1
                else:
                    la["ok"][l], la["size"][l], la["ln"][l] = q
        elif la["armed"]:
            tr["la_miss_short_element"] += 1
        return ok, size, ln

    def step(c):
        E, base = st8["E"], st8["base"]
        c0 = hlen + c * S
        end = c0 + S if c0 + S < clen else clen
        if hst != OK or base >= n or E >= end:
            ent[c] = SKIP
            if hst == OK and base < n and E < BAD:
                tr["skip_chunk_inside_element"] += 1
            return
        ent[c], base_of[c] = E, base
        el = (E - c0) & M64
        if el < 64:
            tr["lookup_entry_%d" % el] += 1
            st8["base"], st8["E"] = base + O[c][el], X[c][el]
            st8["lookups"] += 1
        else:
            tr["walk_entry_%d" % el if el < 66 else "walk_entry_later"] += 1
            x, it = E, 0
            while x < end and base < n:
                it += 1
                if it > S:
                    raise Stall("step")
                ok, size, ln = parse_la(x)
                if not ok:
                    x = (clen + 1) & M64 if parent else BAD
                    break
                base += ln
                x += size
            st8["base"], st8["E"] = base, x

    demand, kinds = False, []
    for b in range(nblk):
        c0 = hlen + b * NBLK * S
        E, base = st8["E"], st8["base"]
        el = (E - c0) & M64
        fast = False
        if hst == OK and base < n and el < 64:
            f = F[b][el]
            if f != ESC64 and base + (f >> 8) < n:
                fast = True
                BE[b], BB[b] = E, base
                st8["base"], st8["E"] = base + (f >> 8), c0 + NBLK * S + (f & 0xFF)
                kinds.append(("fast", 0))
            elif f != ESC64:
                tr["block_with_N_not_fast"] += 1
            elif NBLK * b + NBLK <= nch:
                tr["block_slow_esc_inside"] += 1
        elif hst == OK and base < n and el < S and NBLK * b + NBLK <= nch:
            tr["block_slow_entry_64_or_later"] += 1
        if not fast:
            BE[b] = SKIP
            st8["lookups"] = 0
            cb, ce = NBLK * b, min(NBLK * b + NBLK, nch)
            if demand:
                c, it = cb, 0
                while c < ce:
                    it += 1
                    if it > 2 * NBLK:
                        raise Stall("demand")
                    cc0 = hlen + c * S
                    E = st8["E"]
                    if hst == OK and st8["base"] < n and E >= cc0 + S and E < clen:
                        cn = min((E - hlen) // S, ce)
                        for i in range(c, cn):
                            ent[i] = SKIP
                        tr["demand_skip_%d" % (cn - c) if cn - c in (1, 2, 63) else "demand_skip_other"] += 1
                        c = cn
                        continue
                    step(c)
                    c += 1
            else:
                for c in range(cb, ce):
                    step(c)
            kinds.append(("demand" if demand else "prefetch", st8["lookups"]))
            if demand and st8["lookups"] >= KDEMAND:
                tr["demand_block_meets_short_elements"] += 1
            demand = st8["lookups"] < KDEMAND
    for i, (k, lk) in enumerate(kinds):
        tr["block_" + k] += 1
        if i and k == "prefetch" and lk >= KDEMAND and kinds[i - 1][0] == "prefetch" and kinds[i - 1][1] >= KDEMAND:
            tr["prefetch_8_lookups_twice"] += 1
        if i and k == "demand" and kinds[i - 1][0] != "fast" and kinds[i - 1][1] < KDEMAND:
            tr["few_lookups_then_demand"] += 1
        if 0 < i < len(kinds) - 1 and k != "fast" and kinds[i - 1][0] == "fast" and kinds[i + 1][0] == "fast":
            tr["fast_slow_fast"] += 1
    carried = st8["base"]

    # ---- K5b3 ----
    for b in range(nblk):
        if BE[b] == SKIP:
            continue
        c0 = hlen + b * NBLK * S
        el, base = (BE[b] - c0) & M32, BB[b]
        for j in range(NBLK):
            ent[NBLK * b + j], base_of[NBLK * b + j] = c0 + j * S + el, base
            tr["fill_chunk"] += 1
            w = P[NBLK * b + j][el]
            base, el = base + (w >> 8), w & 0xFF

    # ---- K5c, K5d ----
    offs, cst, fin = {}, [OK] * nch, None

    def hook(h):
        ia, c0, ex, es = h["ia"], h["c0"], h["e_x"], h["e_size"]
        if h["restaged"]:
            tr["k5c_restage"] += 1
        if len(ex) == 32 and all(v == 2 for v in es):
            tr["k5c_batch_of_32_two_byte_elements"] += 1
        if es[0] >= 64:
            tr["k5c_batch_first_element_64_or_more"] += 1
        for k in range(len(ex)):
            a = c0 + ex[k]
            d = ia + WIN - a
            if 1 <= d <= 5:
                tr["k5c_window_edge_%s_%d" % (par.kind(a), d)] += 1
            if k < h["nexec"]:
                d = c0 + S - a  # header bytes before the chunk end
                if 1 <= d <= 5 and a + d <= clen:
                    kd = par.kind(a)
                    if d <= _HB[kd]:
                        tr["chunk_edge_%s_%d" % (kd, d)] += 1
                if (a + es[k] - hlen) // S - (a - hlen) // S >= 4:
                    tr["literal_covers_three_chunks"] += 1
        for k, what in h["wrote"]:
            a, ln, kd = c0 + ex[k], h["e_len"][k], par.kind(c0 + ex[k])[0]
            if what == "end":
                nxt = a + es[k]
                tr["end_on_boundary_successor_in_%s_chunk" % ("next" if (nxt - hlen) % S == 0 else "same")] += 1
            else:
                skip = (h["e_op"][k] // B + 1) * B - h["e_op"][k]
                if skip == 1:
                    tr["straddle_%s_by_1" % kd] += 1
                if skip == ln - 1:
                    tr["straddle_%s_by_len_minus_1" % kd] += 1
        if [w for _, w in h["wrote"]].count("straddle") >= 3:
            tr["straddle_three_boundaries"] += 1
        if h["er"] == OVERRUN and h["nexec"] >= 2 and any(k < h["nexec"] - 1 for k, _ in h["wrote"]):
            tr["overrun_not_first_with_entry_before"] += 1

    for c in range(nch):
        x = ent[c]
        if x == SKIP:
            continue
        c0 = hlen + c * S
        end_rel = (S if c0 + S < clen else (clen - c0) & M64) & M32
        assert c0 <= x < c0 + end_rel <= clen
        st, x, op = k5_model.batched(s, c0, x - c0, c0 + end_rel, base_of[c], n, offs, parse_at=par, win=WIN,
                                     ia=x & ~3, hook=hook)
        if st == OK and op == n:
            offs[units] = fin = x
            if (x - hlen) % S == 0 and x == clen:
                tr["last_element_ends_on_chunk_end"] += 1
            if x < clen:
                tr["bytes_after_N"] += 1
        if st == OK and op < n and x >= clen:
            st = TRUNC
        cst[c] = st
    if not parent and hst == OK and n == 0 and max_units > 0:
        offs[0] = fin = hlen
    st = hst
    if st == OK and units >= max_units:
        st = CAPACITY
    if st == OK:
        bad = [v for v in cst if v != OK]
        if len(bad) >= 2 and bad[0] != bad[-1]:
            tr["errors_in_two_chunks"] += 1
        if bad:
            st = bad[0]
    if st == OK and carried < n:
        st = TRUNC
    if st == OK and units:
        offs[0] = 0
    if st == OK and tr["la_lane_past_clen"]:
        tr["la_lanes_past_clen_chain_clean"] += 1
    return dict(status=st, n=n, units=units, ent=ent, base=base_of, tr=tr,
                offsets=[offs.get(i) for i in range(units + 1)] if st == OK else None)


# ---------------------------------------------------------------------------
# the inputs: name -> (stream, element list or None)
# ---------------------------------------------------------------------------
def _either_hlen(gen):
    for hlen in (3, 4):
        try:
            return gen(hlen)
        except ValueError:
            pass
    raise AssertionError("no preamble length fits")


def length_stream(hlen, clen, seed):
    sb = SB(hlen, seed)
    if hlen >= 3:
        n = None
        if hlen == 4:
            sb.lit(64, 1)
            while sb.op < (1 << 21) + 64 and sb.pos + 3 <= clen - 200:
                sb.copy(64, 2, off=64)
            if sb.op < 1 << 21:  # m = 4: declared, never reached (TRUNCATED)
                n = 1 << 21
        sb.fill_to(clen)
        return sb.finish(n), (sb.elems if n is None else None)
    sb.out_to(100 if hlen == 1 else 9000)
    sb.raw(sb.rng.bytes(clen - sb.pos))  # bytes after N
    return sb.finish(), sb.elems


def gen_lengths():
    out = {"len_65535": lambda: length_stream(3, 65535, 1), "len_65536": lambda: length_stream(3, 65536, 2)}
    for hlen in (1, 2, 3, 4):
        for m in (4, 65):
            for d in sorted({0, 1, hlen - 1, hlen, hlen + 1, 16383}):
                out["len_h%d_m%d_d%d" % (hlen, m, d)] = functools.partial(length_stream, hlen, m * S + d,
                                                                          100 * hlen + m + d)
    return out


HANG_INPUTS = ["len_h%d_m%d_d%d" % (h, m, h - 1) for h in (2, 3, 4) for m in (4, 65)]


def gen_chunk_edges(hlen):
    sb = SB(hlen, 11)
    sb.lit(500)
    cases = [("L", 0, 1, e) for e in (1, 30, 60)]
    for w in (1, 2, 3, 4):
        cases += [("L", w, k, e) for k in range(1, w + 2) for e in (1, 62, 63, 64, 65, S + 1)
                  if 1 <= k + e - (1 + w) <= 256 ** w]  # (a header cut after k bytes enters at byte 1 + w - k at least)
    cases += [("C", kind, k, 0) for kind, hb in ((1, 2), (2, 3), (4, 5)) for k in range(1, hb + 1)]
    cases += [("Lend", w, 0, 0) for w in range(5)]  # ends on the chunk end: entry byte 0
    for what, w, k, e in cases:
        cend = hlen + ((sb.pos - hlen) // S + 1) * S
        if cend - sb.pos < 400:
            cend += S
        if what == "L":
            sb.fill_to(cend - k)
            sb.lit(k + e - (1 + w), w)
            assert sb.pos == cend + e
        elif what == "C":
            sb.fill_to(cend - k)
            sb.copy(5, w)
        else:
            sb.fill_to(cend - (1 + w) - 7)
            sb.lit(7, w)
            assert sb.pos == cend
    cend = hlen + ((sb.pos - hlen) // S + 2) * S
    sb.fill_to(cend - 100)
    sb.lit(100 + 3 * S + 50, 3)  # covers three whole chunks
    sb.fill_to(cend + 4 * S + 1000)
    return sb.finish(), sb.elems


def gen_conv_late(hlen):
    sb = SB(hlen, 12)
    sb.lit(700)
    sb.fill_to(hlen + S)
    for _ in range(210):  # 01 01 at a chunk start: the even and odd chains pass two checkpoints apart
        sb.copy(4, 1, off=1)
    sb.fill_to(hlen + 5 * S - 300)
    return sb.finish(), sb.elems


def periodic(unit, elen, count):
    lit = bytes(range(200)) * 3
    n = len(lit) + elen * count
    return varint(n) + bytes([61 << 2, 599 & 0xFF, 599 >> 8]) + lit + bytes(unit) * count, None


def gen_esc_out24():
    sb = SB(4, 13)
    sb.fill_to(4 + 700)
    sb.raw(bytes([63 << 2]) + (1 << 24).to_bytes(4, "little") + sb.rng.bytes(70 << 10))  # declares 2^24 + 1 bytes
    return sb.finish(sb.op + (1 << 24) + 1), None


def gen_blocks_fsf(hlen):
    sb = SB(hlen, 21)
    sb.fill_to(hlen + 64 * S + 10)  # block 0: fast
    sb.fill_to(hlen + 84 * S - 50)
    sb.lit_size(250)  # block 1: one Esc (an exit 200 bytes into the next chunk)
    sb.fill_to(hlen + 128 * S + 5)
    sb.fill_to(hlen + 192 * S + 7)  # block 2: fast
    sb.fill_to(hlen + 194 * S + 100)
    return sb.finish(), sb.elems


def gen_blocks_e64n(hlen):
    sb = SB(hlen, 22)
    sb.fill_to(hlen + 64 * S - 30)
    sb.lit_size(130)  # block 0 exits 100 bytes into block 1: Esc in its last chunk
    sb.fill_to(hlen + 128 * S + 3)  # block 1: no Esc of its own, entered at byte 100
    sb.fill_to(hlen + 158 * S + 77)  # block 2: N is reached in it ...
    n = sb.op
    sb.counted = False
    sb.fill_to(hlen + 194 * S + 9)  # ... and well-formed elements go on after N
    return sb.finish(n), sb.elems


def gen_blocks_demand(hlen):
    sb = SB(hlen, 23)
    sb.lit(100)
    while sb.pos < hlen + 63 * S - 61000:  # block 0: 60,000-byte literals, few lookups
        sb.lit(60000)
    sb.fill_to(hlen + 63 * S + 200, 3000, 6000)
    sb.lit_size(64 * S + 5000)  # block 1 (demand): chunks 64..126 jumped over
    sb.lit_size(2 * S)  # from chunk 127 over chunk 128 (block 2, demand)
    sb.lit_size(3 * S)  # from chunk 129 over chunks 130 and 131
    sb.fill_to(hlen + 194 * S + 50)  # short elements again: lookups on demand
    return sb.finish(), sb.elems


def gen_lookahead(hlen):
    sb = SB(hlen, 24)
    sb.lit(300)
    sb.fill_to(hlen + S - 40)
    sb.lit_size(140)  # chunk 1 is entered at byte 100: walked
    for _ in range(30):
        sb.lit(62, 1)  # size 64
    for _ in range(8):
        sb.lit(5000)
    sb.lit(3000)  # another size: a miss
    sb.fill_to(sb.pos + 2000, 2, 12)  # short elements
    sb.lit(9000)
    for _ in range(3):
        sb.lit(5000)  # the lookahead lanes of this run parse past clen
    return sb.finish(), sb.elems


def gen_k5c_short(hlen):
    sb = SB(hlen, 25)
    sb.lit(100)
    ks = sb.rng.integers(0, 10, 400_000).tolist()
    while sb.pos < 900_000:
        k = ks.pop()
        if k < 5:
            sb.lit(1, k)
        elif k == 5:
            sb.copy(int(sb.rng.integers(4, 12)), 1)
        elif k < 8:
            sb.copy(int(sb.rng.integers(1, 4)), 2)
        else:
            sb.copy(int(sb.rng.integers(1, 4)), 4)
        if sb.rng.integers(0, 2000) == 0:
            for _ in range(200):  # two-byte elements only
                if sb.rng.integers(0, 2):
                    sb.lit(1, 0)
                else:
                    sb.copy(4, 1)
    return sb.finish(), sb.elems


def gen_k5c_bound(overrun):
    def gen(hlen):
        sb = SB(hlen, 26)
        sb.lit(200)
        sb.fill_out(B - 300)
        sb.sync(sb.pos + 900, B, "lit")  # ends on 65,536; the successor in the same chunk
        assert (sb.pos - hlen) % S
        sb.fill_out(2 * B - 24000)
        e = hlen + ((sb.pos + 3000 - hlen) // S + 1) * S
        sb.sync(e, 2 * B, "copy")  # ends on 131,072 and on a chunk end
        sb.fill_out(3 * B)
        sb.out_to(3 * B - 1)
        sb.copy(30)
        sb.fill_out(4 * B)
        sb.out_to(4 * B - 29)
        sb.copy(30)
        sb.fill_out(5 * B)
        sb.out_to(5 * B - 1)
        sb.lit(40)
        sb.fill_out(6 * B)
        sb.out_to(6 * B - 39)
        sb.lit(40, 1)
        sb.fill_out(7 * B)
        sb.out_to(7 * B - 10)
        sb.copy(20)  # straddles 458,752
        sb.lit(5)
        sb.copy(30)
        return sb.finish(sb.op - 1 if overrun else None), (None if overrun else sb.elems)
    return gen


def gen_lit200k(hlen):
    sb = SB(hlen, 27)
    sb.lit(1000)
    sb.lit(200_000, 3)
    sb.fill_to(280_000)
    return sb.finish(), sb.elems


def gen_n_mult(d):
    def gen(hlen):
        sb = SB(hlen, 28 + d)
        sb.fill_out(2 * B + d)
        sb.out_to(2 * B + d)
        return sb.finish(), sb.elems
    return gen


@functools.lru_cache(maxsize=None)
def gen_cuts():
    out = {}
    for where, p in (("edge", 3 + 4 * S - 2), ("mid", 3 + 4 * S + 5000)):
        sb = SB(3, 30)
        sb.fill_to(p)
        sb.lit(300, 4)
        s = sb.finish()
        for j in (1, 2, 3, 4, 5, 155):
            out["cut_%s_%d" % (where, j)] = (s[:p + j], None)
    return out


@functools.lru_cache(maxsize=None)
def gen_unsup():
    sb = SB(4, 31)
    sb.out_to(B - 10)
    sb.lit((1 << 24) + 70000)
    sb.fill_to(sb.pos + 3000)
    s = sb.finish()
    return {"unsup_17m": (s, None), "unsup_17m_cut_tail": (s[:-7], None)}


def _generators():
    g = gen_lengths()
    for name, gen in (("chunk_edges", gen_chunk_edges), ("conv_late", gen_conv_late), ("blocks_fsf", gen_blocks_fsf),
                      ("blocks_e64n", gen_blocks_e64n), ("blocks_demand", gen_blocks_demand),
                      ("lookahead", gen_lookahead), ("k5c_short", gen_k5c_short), ("k5c_bound", gen_k5c_bound(False)),
                      ("st_overrun", gen_k5c_bound(True)), ("lit200k", gen_lit200k), ("n_mult_-1", gen_n_mult(-1)),
                      ("n_mult_+0", gen_n_mult(0)), ("n_mult_+1", gen_n_mult(1))):
        g[name] = functools.partial(_either_hlen, gen)
    g["period_0101"] = lambda: periodic((1, 1), 4, 40_600)
    g["period_020202"] = lambda: periodic((2, 2, 2), 1, 27_000)
    g["esc_out24"] = gen_esc_out24
    for w in ("edge", "mid"):
        for j in (1, 2, 3, 4, 5, 155):
            g["cut_%s_%d" % (w, j)] = functools.partial(lambda k: gen_cuts()[k], "cut_%s_%d" % (w, j))
    g["n0"] = lambda: (b"\x00" + np.random.default_rng(40).bytes(B), None)
    g["hdr10"] = lambda: (b"\xff" * 10 + np.random.default_rng(41).bytes(B), None)
    for k in ("unsup_17m", "unsup_17m_cut_tail"):
        g[k] = functools.partial(lambda k: gen_unsup()[k], k)
    return g


_GEN = _generators()


class _Lazy(dict):
    """name -> (stream, element list or None), built on first use."""

    def __missing__(self, name):
        v = self[name] = _GEN[name]()
        return v


_INPUTS = _Lazy()


def inputs():
    return _INPUTS


NAMES = (["len_65535", "len_65536"]
         + ["len_h%d_m%d_d%d" % (h, m, dd) for h in (1, 2, 3, 4) for m in (4, 65)
            for dd in sorted({0, 1, h - 1, h, h + 1, 16383})]
         + ["chunk_edges", "conv_late", "period_0101", "period_020202", "esc_out24", "blocks_fsf", "blocks_e64n",
            "blocks_demand", "lookahead", "k5c_short", "k5c_bound", "st_overrun", "lit200k", "n_mult_-1", "n_mult_+0",
            "n_mult_+1"]
         + ["cut_%s_%d" % (w, j) for w in ("edge", "mid") for j in (1, 2, 3, 4, 5, 155)]
         + ["n0", "hdr10", "unsup_17m", "unsup_17m_cut_tail"])
MISALIGNED = ["chunk_edges", "k5c_bound", "len_h3_m4_d2"]


@functools.lru_cache(maxsize=None)
def expected(name, max_units=MAX_UNITS):
    return k5_serial(inputs()[name][0], max_units)


# the edges of the issue's list -> the model's trace keys (all must be reached)
_HB = {"L1": 1, "L2": 2, "L3": 3, "L4": 4, "L5": 5, "C1": 2, "C2": 3, "C4": 5}  # header bytes per element kind
_WIN_EDGES = ["%s_%s_%d" % (w, k, d) for w in ("k5c_window_edge", "chunk_edge") for k, hb in _HB.items()
              for d in range(1, hb + 1)]
EDGES = ["k5a_start_at_or_past_clen", "k5a_short_last_chunk", "k5a_merged_at_checkpoint_1",
         "k5a_merged_after_checkpoint_2", "k5a_never_merged", "esc_output_2^24", "esc_last_full_chunk",
         "esc_exit_past_byte_63", "lookup_entry_0", "lookup_entry_1", "lookup_entry_62", "lookup_entry_63",
         "walk_entry_64", "walk_entry_65", "skip_chunk_inside_element", "block_fast", "block_prefetch", "block_demand",
         "block_slow_entry_64_or_later", "block_slow_esc_inside", "fast_slow_fast", "fill_chunk",
         "block_with_N_not_fast", "prefetch_8_lookups_twice", "few_lookups_then_demand", "demand_skip_1",
         "demand_skip_2", "demand_skip_63", "demand_block_meets_short_elements", "la_hit", "la_miss_other_size",
         "la_miss_short_element", "la_lanes_past_clen_chain_clean", "k5c_restage",
         "k5c_batch_of_32_two_byte_elements", "k5c_batch_first_element_64_or_more",
         "end_on_boundary_successor_in_same_chunk", "end_on_boundary_successor_in_next_chunk", "straddle_C_by_1",
         "straddle_C_by_len_minus_1", "straddle_L_by_1", "straddle_L_by_len_minus_1", "straddle_three_boundaries",
         "overrun_not_first_with_entry_before", "last_element_ends_on_chunk_end", "errors_in_two_chunks",
         "literal_covers_three_chunks", "bytes_after_N"] + _WIN_EDGES


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_names_are_the_inputs():
    assert sorted(NAMES) == sorted(_GEN)
    for name in HANG_INPUTS + MISALIGNED:
        assert name in _GEN
    for name in HANG_INPUTS:
        s = inputs()[name][0]
        hlen = next(k for k in range(10) if not s[k] & 0x80) + 1
        assert hlen >= 2 and len(s) >= B and (len(s) - (hlen - 1)) % S == 0


def test_model_stalls_with_the_parents_arithmetic():
    s = inputs()["len_h3_m4_d2"][0]
    assert len(s) == 65538 and s[2] < 0x80 <= s[1]
    with pytest.raises(Stall, match="walk_to: chunk 4 .c0 = 65539, clen = 65538. lane 0 stands at 0"):
        k5p_model(s, parent=True)
    assert k5p_model(s)["status"] == expected("len_h3_m4_d2")[0] == OK
    for name in HANG_INPUTS:
        with pytest.raises(Stall, match="walk_to"):
            k5p_model(inputs()[name][0], parent=True)
    # c0 = clen + 2: the same subtraction wraps to 2^64 - 1 and the parent's loop ends
    k5p_model(inputs()["len_h3_m4_d1"][0], parent=True)


def test_serial_matches_the_element_lists_and_the_oracle():
    for name in NAMES:
        s, elems = inputs()[name]
        st, n, units, offs = expected(name)
        if elems is not None:
            assert st == OK, name
            assert offs == index_from_elems(elems, n), name
            assert len(oracle.decompress(s)) == n, name


def test_statuses():
    want = {"esc_out24": TRUNC, "st_overrun": OVERRUN, "n0": OK, "hdr10": HEADER, "unsup_17m": UNSUP,
            "unsup_17m_cut_tail": UNSUP, "len_h4_m4_d3": TRUNC}
    want.update({"cut_%s_%d" % (w, j): TRUNC for w in ("edge", "mid") for j in (1, 2, 3, 4, 5, 155)})
    for name, st in want.items():
        assert expected(name)[0] == st, name
    assert expected("n0")[1:] == (0, 0, [1])
    u = expected("n_mult_+0")[2]
    assert u == 2 and expected("n_mult_+1")[2] == 3 and expected("n_mult_-1")[2] == 2
    assert k5_serial(inputs()["n_mult_+0"][0], u)[0] == CAPACITY
    assert k5_serial(inputs()["n_mult_+0"][0], u + 1)[0] == OK


def test_inputs_have_their_properties():
    reached = collections.defaultdict(list)
    for name in NAMES:
        s = inputs()[name][0]
        st, n, units, offs = expected(name)
        m = k5p_model(s)
        assert (m["status"], m["n"], m["units"]) == (st, n, units), name
        assert m["offsets"] == offs, name
        if st == OK:
            ent, base = true_chunks(s)
            assert m["ent"] == ent, name
            assert all(b == t for b, t, e in zip(m["base"], base, ent) if e != SKIP), name
        for k in m["tr"]:
            reached[k].append(name)
    for mu in (2, 3):
        assert k5p_model(inputs()["n_mult_+0"][0], max_units=mu)["status"] == k5_serial(inputs()["n_mult_+0"][0], mu)[0]
    for e in EDGES:
        print("%-44s %s" % (e, " ".join(reached[e][:6]) + (" ..." if len(reached[e]) > 6 else "")))
    missing = [e for e in EDGES if not reached[e]]
    assert not missing, missing
    # what the issue ties to one input
    assert "blocks_fsf" in reached["fast_slow_fast"] and "blocks_demand" in reached["demand_skip_63"]
    assert "esc_out24" in reached["esc_output_2^24"] and "lit200k" in reached["straddle_three_boundaries"]
    assert "unsup_17m_cut_tail" in reached["errors_in_two_chunks"]
    assert all("chunk_edges" in reached[e] for e in _WIN_EDGES if e.startswith("chunk_edge"))
    assert "chunk_edges" in reached["literal_covers_three_chunks"]
    assert set(HANG_INPUTS) <= set(reached["k5a_start_at_or_past_clen"])


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
GUARD = 8
SENT = -0x5A5A5A5A5A5A5A5B


def _index(codec, dev, clen, serial, max_units, ptr=None):
    """(code, N, entries) of snappy_amd_index_device; the GUARD entries past max_units must stay."""
    import torch
    offs = torch.full((max_units + GUARD,), SENT, dtype=torch.int64, device="cuda")
    n = ctypes.c_size_t(0)
    codec.set_option(snappy_amd.OPT_SERIAL_INDEX, int(serial))
    try:
        codec._bind_stream()
        rc = snappy_amd.lib().snappy_amd_index_device(codec._h, ctypes.c_void_p(ptr or dev.data_ptr()), clen,
                                                      ctypes.c_void_p(offs.data_ptr()), max_units, ctypes.byref(n))
    finally:
        codec.set_option(snappy_amd.OPT_SERIAL_INDEX, 0)
    got = offs.cpu().numpy()
    assert (got[max_units:] == SENT).all(), "entries past max_units written"
    return rc, n.value, got[:max_units]


def _check_input(codec, name, shift=None, decode=True):
    import torch
    s = inputs()[name][0]
    st, n, units, offs = expected(name)
    mu = units + 1 if st != HEADER else 16
    a = np.frombuffer(s, dtype=np.uint8)
    if shift is None:
        dev, ptr = torch.from_numpy(a.copy()).cuda(), None
    else:
        buf = torch.zeros(len(s) + 8, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        dev = buf[shift:shift + len(s)]
        dev.copy_(torch.from_numpy(a.copy()))
        ptr = buf.data_ptr() + shift
    for serial in (0, 1):
        rc, gn, got = _index(codec, dev, len(s), serial, mu, ptr)
        print(name, "serial" if serial else "K5p", "code", rc, "N", gn, "want", st, n)
        assert rc == st, (name, serial, rc, st)
        assert gn == n, (name, serial)
        if st == OK:
            assert got.astype(np.uint64).tolist() == offs, (name, serial)
    if st == OK and decode and n:
        want = oracle.decompress(s)
        o = torch.from_numpy(np.array(offs, dtype=np.uint64).astype(np.int64)).cuda()
        back = codec.decompress_tensor(dev, o, n, layout=snappy_amd.SINGLE)
        assert back.cpu().numpy().tobytes() == want, name


@pytest.mark.gpu
@pytest.mark.timeout(20)
@pytest.mark.parametrize("name", HANG_INPUTS)
def test_last_chunk_starts_past_the_end(codec, name):
    """clen = m * 16384 + h.len - 1: K5a's last chunk starts at clen + 1."""
    _check_input(codec, name)


@pytest.mark.gpu
@pytest.mark.timeout(20)
@pytest.mark.parametrize("name", [x for x in NAMES if x not in HANG_INPUTS and not x.startswith("unsup")])
def test_index_and_decode(codec, name):
    _check_input(codec, name)


@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", ["unsup_17m", "unsup_17m_cut_tail"])
def test_index_large(codec, name):
    _check_input(codec, name)


@pytest.mark.gpu
@pytest.mark.timeout(20)
@pytest.mark.parametrize("name", MISALIGNED)
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_index_misaligned(codec, name, shift):
    """The stream at a device address of 1, 2 and 3 modulo 4 (K5p indexes an aligned copy)."""
    _check_input(codec, name, shift, decode=False)


@pytest.mark.gpu
@pytest.mark.timeout(20)
def test_capacity(codec):
    import torch
    s = inputs()["n_mult_+0"][0]
    dev = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
    st, n, units, offs = expected("n_mult_+0")
    for serial in (0, 1):
        assert _index(codec, dev, len(s), serial, units)[0] == CAPACITY
        rc, gn, got = _index(codec, dev, len(s), serial, units + 1)
        assert (rc, gn) == (OK, n) and got.astype(np.uint64).tolist() == offs
