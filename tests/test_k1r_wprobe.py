"""K1r / K1r64 W-probe rounds on inputs planted against a model of the round.

After 29 consecutive misses (skip > 64 - LSMIN) the match finder leaves its
lane-space rounds: four probes sit at their closed-form positions p_k = p +
skipsum(skip + k) - skipsum(skip), each lane reads its slot before any insert of
the round, and three rules (`tconf`) stop the round where a lane would read a
slot an earlier lane writes (h_k == h_j, h_k == a_j) or where the two-phase
insert (all a records, then all h records) would leave another owner than the
serial order (a_k == h_j, unless p_j == p_k - 1: the `notdup` mask of steps of
1).  A wrong rule leaves a table the serial reference never has; the output
still round-trips, but it is not the reference's bytes.

In noise a rule only fires on a hash collision between different words.  The
dangerous case is equal words at one small distance inside a long miss run, and
no other input of the suite has that on purpose.  So:

* `w_model` restates k1r_body round by round with the kernel's arithmetic: the
  lane-space rounds (serial probes, but with the window q0, the refresh at
  lane0 + RMIN > 62 and the pending-token count they leave behind) and the W
  round exactly (window reuse test, per-lane sk / pk / inval, h and a, tconf with
  notdup and the zero a lane without a source lane shifts in, the tag-equal hit,
  the first stop f, two-phase inserts, the verified hit or the tag collision of
  lane f, the closed-form advance).  Its tokens must equal `probe_unit`'s serial
  tokens and its size the oracle's, on every unit of every input.  `drop`
  removes one rule (hh, ha, ah), forces notdup to all-ones (nd1) or to zero
  (nd0); only the CPU test uses it.
* every unit is built online against the model: random bytes, and at a W
  round's start (or where lane-space rounds begin) a planter rewrites bytes no
  earlier probe has read, so that one wanted condition holds.  The finished
  unit must replay to the same tokens and the same trace.

Inputs (per unit length, because table size and block end depend on it):

* conf_same: rule x lane distance x lane j in rotation, the 4 bytes copied that
  make word(p_k) or word(p_k - 1) equal word(p_j) or word(p_j - 1), at steps 2,
  3, 4-8 and >= 9 in rotation; an `ah` plant replays the word at the next probe
  position, so the slot's owner shows in an offset.
* conf_diff: the same classes with hash-equal, byte-different words (the last
  two bytes searched): plain; with the tag equal too (a tag collision at lane 0
  right after the conflict stop); and `stale`, where the slot holds an old
  position whose word is the later lane's (the hit a missing hh / ha rule takes).
* dup: a lane-space match ending at window lane 43-47, which makes the next W
  round start at skip 61, 62, 63 or 64 in a window the in-loop refresh moved,
  lanes mixing steps 1 and 2; and a 5-7 byte run of one value across p_{k-1} and
  p_k - 1: at step 1 the dup that must not stop, at step 2 the `ah` conflict that
  must, its word replayed two probes later.
* hits: a W-round hit at each lane and step class, lengths 4-11, 12-63, 64-139
  and >= 259, one match that runs to the unit's end, sources the model says are
  still in the table.
* tails: noise at 48 consecutive lengths: the last rounds are cut by the block
  end at lanes 1, 2 and 3, also where sk >> 5 changes at the cut.
* big_steps (K1r64): 46 KiB of noise (steps >= 52: the window-edge cut at lane
  1, WINDOW_AT at every round, the ring advancing inside W rounds), then hits
  whose sources are far (first 12 KiB, every c % 4), in the edge band, and in
  segment 127.

Forcing notdup to all-ones cannot change the output (a false conflict is retried
as the next round's lane 0): that model mutant must give the same tokens in more
rounds.  The mask's harmful direction is zero (the d1 `ah` rule never fires),
which is nd0.  The W round's `if (pend == 64) flush_tokens()` was never seen
taken: the model records the largest pend at a W-round put_token.

The GPU bar is the oracle's bytes and unit offsets, bit for bit, and the round
trip."""
import collections
import functools
import random

import numpy as np
import pytest

import oracle
import snappy_amd
from test_k1r64_ring import first_resident
from test_k1r_flush_inloop import copy_bytes, literal_bytes, probe_unit

MUL = 0x1E35A7BD
DMAX32, DMAX64, RMIN, LSMIN, W = 13, 12, 2, 4, 4  # SNAPPY_K1R_DMAX, _DMAX64, _RMIN, _LSMIN, _WINDOW
RULES = ("hh", "ha", "ah")
CLASSES = [(r, d) for d in (1, 2, 3) for r in RULES]
DROPS = ("hh", "ha", "ah", "nd1", "nd0")

K1R_INPUTS = ["conf_same", "conf_diff", "dup", "hits", "tails"]
K1R_CHUNKS = [256, 300, 1000, 2048, 4096, 32768]
BIG_INPUTS = K1R_INPUTS + ["big_steps"]
BLOCK, SHORT, SMALLEST64 = 65536, 61001, 32769
BIG_SHAPES = [("single", BLOCK, 4 * BLOCK, BLOCK), ("single", BLOCK, 3 * BLOCK + SHORT, BLOCK),
              ("streams", BLOCK, 4 * BLOCK, BLOCK), ("streams", SHORT, 4 * SHORT, SHORT)]
TAIL_BASES = [2100, 32677]  # 48 consecutive unit lengths from each
TAIL_COUNT = 48
SEEDS = {"conf_same": 510, "conf_diff": 520, "dup": 530, "hits": 540, "tails": 550, "big_steps": 560}
BIG_NOISE = 47104   # big_steps: no plant before this position
BIG_FAR_SRC = 12288


def units_of(chunk: int) -> int:
    return 64 if chunk <= 4096 else 4


def skipsum(m: int) -> int:
    q = m >> 5
    return 16 * q * (q - 1) + (m & 31) * q


def step_class(step: int) -> str:
    for lo, hi in ((1, 1), (2, 2), (3, 3), (4, 8), (9, 16), (17, 45), (46, 51)):
        if lo <= step <= hi:
            return "s%d" % lo if lo == hi else "s%d_%d" % (lo, hi)
    return "s52"


STEP_CLASS = [step_class(s) for s in range(2112)]  # (a 65,536-byte block ends below step 65)


def len_class(n: int) -> str:
    for lo, hi in ((4, 11), (12, 63), (64, 139), (140, 258)):
        if n <= hi:
            return "len_%d_%d" % (lo, hi)
    return "len_259"


def _hash_range(bp, sh: int, lo: int, hi: int):
    """Slot, tag and BE32 of the words at lo .. hi - 1 (the tag: the 8 product bits below the index)."""
    a = np.frombuffer(bp, dtype=np.uint8, count=hi - lo + 3, offset=lo).astype(np.uint32)
    w = (a[:-3] << 24) | (a[1:-2] << 16) | (a[2:-1] << 8) | a[3:]
    pr = w * np.uint32(MUL)
    return (pr >> sh).tolist(), ((pr >> (sh - 8)) & 0xFF).tolist(), w.tolist()


class _Ctx:
    pass


def _call_hook(hook, ctx, kind, p, skip, q0, free):
    ctx.kind, ctx.p, ctx.skip, ctx.q0, ctx.free = kind, p, skip, q0, free
    r = hook(ctx)
    if r:
        lo, hi = max(0, r[0] - 3), min(ctx.L + 1, r[1])
        h_, t_, w_ = _hash_range(ctx.bp, ctx.sh, lo, hi)
        ctx.H[lo:hi] = h_
        ctx.TG[lo:hi] = t_
        ctx.WD[lo:hi] = w_


def _run(bp, L: int, big: bool, drop=None, hook=None):
    """k1r_body on the L bytes of bp (a bytearray, 4 zero bytes after them), round by round."""
    assert drop is None or drop in DROPS
    dmax = DMAX64 if big else DMAX32
    T, lg = 256, 8  # set_htable_size
    while T < 4096 and T < L:
        T <<= 1
        lg += 1
    sh = 32 - lg
    H, TG, WD = _hash_range(bp, sh, 0, L + 1)
    tab = [0] * T  # never-set slots: position 0, whose tag is that of the word at 0
    tr = collections.Counter()
    toks = []
    size = end = 0
    p, skip = 1, 33
    q0, lsw, qsrc = 0, False, "w"
    pend = dkn = 0
    maxpend = -1
    readhi = 3      # the highest byte a decision so far depended on
    seg_hi = 128    # (big) the ring holds segments [seg_hi - 128, seg_hi)
    ctx = None
    if hook:
        ctx = _Ctx()
        ctx.L, ctx.bp, ctx.sh, ctx.tab, ctx.H, ctx.TG, ctx.WD, ctx.big, ctx.dmax = L, bp, sh, tab, H, TG, WD, big, dmax
    cap = 4 * L + 64
    rounds = 0
    while not (L - p < (skip >> 5) + 15):  # is_block_end
        rounds += 1
        if rounds > cap:
            raise RuntimeError("the round loop does not end")
        if skip <= 64 - LSMIN:
            # ---- lane-space rounds: serial probes inside the kernel's rounds and windows
            lane0 = p - q0
            if not lsw or lane0 < 0 or lane0 + RMIN > 62:
                if pend + dkn > 48:
                    pend = 0
                    tr["ls_flush"] += 1
                q0, lsw, qsrc, lane0 = p - 1, True, "entry", 1
                seg_hi = max(seg_hi, (q0 >> 8) + 2)
                if hook:
                    _call_hook(hook, ctx, "ls", p, skip, q0, max(readhi + 1, p + 1))
            inner = 0
            while True:
                inner += 1
                if inner > cap:
                    raise RuntimeError("the lane-space loop does not end")
                pend += dkn
                dkn = 0
                top = min(62, L - 16 - q0)
                if skip > 64 - dmax:  # the round reaches the probe at skip 64 (L - p >= 17 there)
                    hi = lane0 + 64 - skip
                    if hi < 64 and hi > min(62, L - 17 - q0):
                        hi -= 1
                    hi = min(hi, top)
                else:
                    hi = min(lane0 + dmax - 1, top)
                nk = hi - lane0 + 1
                if nk < 1:
                    raise RuntimeError("a lane-space round without a probe")
                f = -1
                for ln in range(lane0, hi + 1):
                    pk = q0 + ln
                    h = H[pk]
                    if TG[tab[h]] == TG[pk]:
                        f = ln
                        break
                    tab[H[pk - 1]] = pk - 1
                    tab[h] = pk
                if f < 0:
                    readhi = max(readhi, q0 + hi + 3)
                    np_ = q0 + lane0 + nk - 1 + ((skip + nk - 1) >> 5)
                    skip += nk
                else:
                    pf = q0 + f
                    c = tab[H[pf]]
                    readhi = max(readhi, pf + 3)
                    if WD[c] == WD[pf]:
                        n = 4
                        while pf + n < L and bp[pf + n] == bp[c + n]:
                            n += 1
                        readhi = max(readhi, min(pf + n, L - 1))
                        toks.append((pf - end, n, pf - c))
                        size += (literal_bytes(pf - end) if pf > end else 0) + copy_bytes(n, pf - c)
                        end = pf + n
                        tab[H[pf]] = pf
                        dkn = 1
                        np_ = end
                        skip = 32
                        seg_hi = max(seg_hi, ((end - 1) >> 8) + 2)
                    else:  # tag collision: a miss
                        tr["ls_tagcoll"] += 1
                        tab[H[pf - 1]] = pf - 1
                        tab[H[pf]] = pf
                        np_ = pf + ((skip + f - lane0) >> 5)
                        skip += f - lane0 + 1
                if np_ <= p:
                    raise RuntimeError("a lane-space round consumed nothing")
                p = np_
                if not (skip <= 64 - LSMIN and p <= L - 16):
                    break
                lane0 = p - q0
                if lane0 + RMIN > 62:
                    if pend + dkn > 48:
                        pend = 0
                        tr["ls_flush"] += 1
                    q0, qsrc, lane0 = p - 1, "inloop", 1
                    seg_hi = max(seg_hi, (q0 >> 8) + 2)
            pend += dkn
            dkn = 0
            continue
        # ---- W-probe round
        tr["wround"] += 1
        lsw = False
        if p - 1 < q0 or p + 12 > q0 + 64:
            q0, qsrc = p - 1, "w"
            tr["win_move"] += 1
            if big and (q0 >> 8) + 2 > seg_hi:
                seg_hi = (q0 >> 8) + 2
                tr["ring_adv_w"] += 1
        else:
            tr["win_reuse"] += 1
            if qsrc != "w":
                tr["reuse_ls_window"] += 1
            if qsrc == "inloop":
                tr["reuse_inloop_window"] += 1
        if hook:
            _call_hook(hook, ctx, "w", p, skip, q0, max(readhi + 1, p + 3))
        tr["step_" + STEP_CLASS[skip >> 5]] += 1
        if 61 <= skip <= 64:
            tr["start%d" % skip] += 1
        s0 = skipsum(skip)
        pks, hs, as_, es, inv = [], [], [], [], []
        for k in range(W):
            sk = skip + k
            pk = p + skipsum(sk) - s0
            i_be = (L - pk) - ((sk >> 5) + 15) < 0
            i_we = (q0 + 64) - (pk + 12) < 0
            ik = 1 if i_we else (2 if i_be else 0)  # (named by the window's edge where both hold)
            pos = pk if ik == 0 else q0 + 1  # an invalid lane reads window lane 1
            pks.append(pk)
            hs.append(H[pos])
            as_.append(H[pos - 1])
            es.append(tab[H[pos]])
            inv.append(ik)
        f, why, kinds = W, "all_miss", ()
        for k in range(W):
            sk = skip + k
            if inv[k]:
                f, why = k, ("blockend%d" if inv[k] == 2 else "winedge%d") % k
                if inv[k] == 2 and k and (sk >> 5) != ((sk - 1) >> 5):
                    tr["blockend_skcross"] += 1
                break
            pk = pks[k]
            found = []
            if k:
                notdup = ((sk - 1) >> 5) != 1
                if drop == "nd1":
                    notdup = True
                elif drop == "nd0":
                    notdup = False
                if not notdup:
                    tr["dup_pass"] += 1
                for d in (1, 2, 3):
                    j = k - d
                    hj, aj = (hs[j], as_[j]) if j >= 0 else (0, 0)  # no source lane: 0 is shifted in
                    if hs[k] == hj and drop != "hh":
                        found.append(("hh", d, j, j >= 0 and WD[pk] == WD[pks[j]]))
                    if hs[k] == aj and drop != "ha":
                        found.append(("ha", d, j, j >= 0 and WD[pk] == WD[pks[j] - 1]))
                    if as_[k] == hj and (d > 1 or notdup) and drop != "ah":
                        found.append(("ah", d, j, j >= 0 and WD[pk - 1] == WD[pks[j]]))
            if found:
                f, why, kinds = k, "conf%d" % k, found
                break
            if TG[es[k]] == TG[pk]:
                f, why = k, "hit"
                break
        for rule, d, j, same in kinds:
            if j < 0:
                tr["zero_conf"] += 1
            else:
                tr[("same_" if same else "diff_") + rule + str(d)] += 1
                if same and rule == "ah" and d == 1:
                    tr["same_ah1_step2" if ((skip + f - 1) >> 5) == 2 else "same_ah1_other"] += 1
        # two-phase inserts of the exact misses: all a records, then all h (the highest lane wins)
        for k in range(f):
            tab[as_[k]] = pks[k] - 1
        for k in range(f):
            tab[hs[k]] = pks[k]
        last = min(f, W - 1)
        if inv[last]:
            last -= 1
        if last >= 0:
            readhi = max(readhi, pks[last] + 3)
        next_f = f
        if why == "hit":
            pf, c = pks[f], es[f]
            cls = STEP_CLASS[(skip + f) >> 5]
            if WD[c] == WD[pf]:
                n = 4
                while pf + n < L and bp[pf + n] == bp[c + n]:
                    n += 1
                readhi = max(readhi, min(pf + n, L - 1))
                tr["hit%d" % f] += 1
                tr["hit%d_%s" % (f, cls)] += 1
                tr[len_class(n)] += 1
                if pf + n == L:
                    tr["len_to_L"] += 1
                if big:
                    fr = first_resident(pf)
                    if c + 512 <= fr:
                        tr["wfar"] += 1
                        tr["wfar_c%d" % (c & 3)] += 1
                    elif c >= fr:
                        tr["wwrap" if (c >> 8) & 127 == 127 else "wres"] += 1
                    elif c >= fr - 512:
                        tr["wedge"] += 1
                if pend == 64:
                    tr["w_flush"] += 1
                    pend = 0
                maxpend = max(maxpend, pend)
                pend += 1
                toks.append((pf - end, n, pf - c))
                size += (literal_bytes(pf - end) if pf > end else 0) + copy_bytes(n, pf - c)
                end = pf + n
                tab[hs[f]] = pf
                skip = 32
                p = end
                seg_hi = max(seg_hi, ((end - 1) >> 8) + 2)
                continue
            tr["tagcoll%d" % f] += 1
            if f == 0 and tr["last_conf_round"] == tr["wround"] - 1:
                tr["tagcoll0_after_conf"] += 1
            tab[as_[f]] = pf - 1
            tab[hs[f]] = pf
            next_f = f + 1
        else:
            tr[why] += 1
            if why.startswith("conf"):
                tr["last_conf_round"] = tr["wround"]
        if next_f == 0:
            raise RuntimeError("a W round consumed nothing")
        p = p + next_f if skip + next_f <= 64 else p + skipsum(skip + next_f) - s0
        skip += next_f
    size += literal_bytes(L - end) if L > end else 0
    del tr["last_conf_round"]
    tr["max_pend_w"] = maxpend
    return toks, size, tr


def w_model(b: bytes, big: bool, drop=None):
    """Tokens (gap, length, offset), encoded size and trace counters of one unit."""
    return _run(bytearray(b) + bytes(4), len(b), big, drop)


# ---- planters: called by the model with the state at a round's start

TARGETS = {"conf_same": (2, 3, 4, 2, 3, 4, 2, 9), "conf_diff": (2, 3, 4, 2, 3, 4, 2, 9),
           "hits": (2, 3, 4, 9, 2, 17, 3, 4), "dup": (2,), "big_steps": (2, 3, 2, 4)}
LEN_CLASSES = ((4, 11), (12, 63), (64, 139), (259, 400))


class Planter:
    def __init__(self, kind: str, L: int, big: bool, seed):
        self.kind, self.L, self.big = kind, L, big
        self.r = random.Random(repr(seed))
        self.n = seed[2]  # plants made (the rotations start elsewhere in every unit)
        self.fails = 0    # rounds at which the wanted plant did not fit
        self.jrot = 0
        self.hold = 0     # no plant before this position (a laid-out plan is still running)
        self.cycle = 5 * seed[2]  # dup / step-1 plans made
        self.to_L = False
        self.wr = []      # bytes written by the current attempt: (index, old value)

    # -- byte edits that can be undone
    def put(self, ctx, x: int, v: int) -> bool:
        if ctx.bp[x] == v:
            return True
        if x < ctx.free or x >= self.L:
            return False
        self.wr.append((x, ctx.bp[x]))
        ctx.bp[x] = v
        return True

    def copy(self, ctx, tgt: int, src: int, n: int) -> bool:
        for i in range(n):
            if not self.put(ctx, tgt + i, ctx.bp[src + i]):
                return False
        return True

    def undo(self, ctx):
        for x, v in reversed(self.wr):
            ctx.bp[x] = v
        self.wr = []

    def done(self):
        lo = min(x for x, _ in self.wr)
        hi = max(x for x, _ in self.wr) + 1
        self.wr = []
        return lo, hi

    @staticmethod
    def word(ctx, q: int) -> bytes:
        return bytes(ctx.bp[q:q + 4])

    def hash_of(self, ctx, q: int):
        pr = (int.from_bytes(ctx.bp[q:q + 4], "big") * MUL) & 0xFFFFFFFF
        return pr >> ctx.sh, (pr >> (ctx.sh - 8)) & 0xFF

    def source(self, ctx, lo: int, hi: int, room: int, mod4=None):
        """A position in [lo, hi) that the table still holds, with room bytes after it below ctx.p."""
        hi = min(hi, ctx.p - room - 4)
        if hi <= lo:
            return None
        for _ in range(96):
            s = self.r.randrange(lo, hi)
            if mod4 is not None:
                s = (s & ~3) | mod4
            if lo <= s < hi and ctx.tab[ctx.H[s]] == s:
                return s
        return None

    def search(self, ctx, q: int, slot: int, tag, other: bytes) -> bool:
        """Rewrite bytes q + 2, q + 3 so that the word at q falls into slot (with tag, if given) and is not other."""
        if q + 2 < ctx.free or q + 4 > self.L:
            return False
        base = (ctx.bp[q] << 24) | (ctx.bp[q + 1] << 16)
        w = np.uint32(base) + np.arange(65536, dtype=np.uint32)
        pr = w * np.uint32(MUL)
        ok = (pr >> ctx.sh) == slot
        if tag is not None:
            ok &= ((pr >> (ctx.sh - 8)) & 0xFF) == tag
        ok &= w != np.uint32(int.from_bytes(other, "big"))
        idx = np.flatnonzero(ok)
        if idx.size == 0:
            return False
        v = int(idx[self.r.randrange(idx.size)])
        return self.put(ctx, q + 2, v >> 8) and self.put(ctx, q + 3, v & 0xFF)

    # -- the round's lanes
    def lanes(self, ctx, n: int = 9):
        s0 = skipsum(ctx.skip)
        return [ctx.p + skipsum(ctx.skip + k) - s0 for k in range(n)]

    def valid(self, ctx, P, k: int) -> bool:
        return self.L - P[k] >= ((ctx.skip + k) >> 5) + 15 and P[k] + 12 <= ctx.q0 + 64

    def due(self, ctx) -> bool:
        tg = TARGETS[self.kind]
        t = tg[self.n % len(tg)]
        step = ctx.skip >> 5
        if step >= t:
            return True
        return ctx.p + skipsum(32 * t) - skipsum(ctx.skip) + 48 > self.L  # out of reach: plant now

    def __call__(self, ctx):
        if ctx.p < self.hold:
            return None
        self.wr = []
        if ctx.kind == "ls":
            if self.kind == "dup" or (self.kind == "hits" and self.n % 5 == 4):
                return self.ls_plan(ctx)
            return None
        if self.kind == "big_steps" and ctx.p < BIG_NOISE:
            return None
        if self.kind == "dup":
            return self.hit(ctx, k=1, ln=self.r.randrange(4, 9))
        if ctx.skip < 64 or not self.due(ctx):
            return None
        if self.kind in ("conf_same", "conf_diff"):
            r = self.conf(ctx)
        else:
            r = self.hit(ctx)
        if r is None:
            self.fails += 1
            if self.fails >= 8:  # this one does not fit here (block end, window edge): the next
                self.fails = 0
                self.n += 1
        return r

    def conf(self, ctx):
        rule, d = CLASSES[self.n % 9]
        P = self.lanes(ctx)
        same = self.kind == "conf_same"
        variant = ("plain", "stale", "tag", "stale")[(self.n // 9) % 4]
        if variant == "stale" and rule == "ah":
            variant = "plain"
        for dj in range(W - d):
            j = (self.jrot + dj) % (W - d)
            k = j + d
            if not (self.valid(ctx, P, j) and self.valid(ctx, P, k)):
                continue
            src = P[j] if rule != "ha" else P[j] - 1
            tgt = P[k] if rule != "ah" else P[k] - 1
            if rule == "ah" and src == tgt:
                continue
            ok = False
            if same:
                ok = self.copy(ctx, tgt, src, 4) and self.word(ctx, tgt) == self.word(ctx, src)
            elif variant == "stale":
                s = self.source(ctx, 1, ctx.p, 8)
                if s is not None and tgt >= src + 4:
                    ok = (self.search(ctx, src, ctx.H[s], None, self.word(ctx, s)) and self.copy(ctx, tgt, s, 4)
                          and self.hash_of(ctx, src)[0] == ctx.H[s] and self.word(ctx, src) != self.word(ctx, s))
            else:
                slot, tag = self.hash_of(ctx, src)
                ok = self.search(ctx, tgt, slot, tag if variant == "tag" else None, self.word(ctx, src))
                if not ok and variant == "tag":
                    self.undo(ctx)
                    ok = self.search(ctx, tgt, slot, None, self.word(ctx, src))
                ok = ok and self.hash_of(ctx, src)[0] == slot
            if ok and rule == "ah":
                # replay the word at the next probe position: the slot's owner shows in the offset
                mark = len(self.wr)
                if not (self.copy(ctx, P[k + 1], tgt, 4) and self.word(ctx, P[k + 1]) == self.word(ctx, tgt)
                        and (not same or self.word(ctx, tgt) == self.word(ctx, src))
                        and (same or self.hash_of(ctx, tgt)[0] == self.hash_of(ctx, src)[0])):
                    for x, v in reversed(self.wr[mark:]):
                        ctx.bp[x] = v
                    del self.wr[mark:]
            if ok and self.wr:
                self.n += 1
                self.jrot += 1
                self.fails = 0
                return self.done()
            self.undo(ctx)
        return None

    def hit(self, ctx, k=None, ln=None):
        P = self.lanes(ctx)
        if k is None:
            k = (self.n + self.n // 8) % 4  # (the step targets repeat every 8 plants)
        m = k if P[k] >= ctx.free else k + 4
        if k == 0 and m == 4:  # the next round's lane 0: where this round ends if all its lanes miss
            m = min([j for j in (1, 2, 3) if not self.valid(ctx, P, j)] + [4])
        if P[m] < ctx.free or (m == k and self.kind != "big_steps" and not self.valid(ctx, P, k)):
            return None  # (a lane past the window's edge would be found as the next round's lane 0)
        if ln is None:
            lo, hi = LEN_CLASSES[(self.n // 2 + self.n // 32) % 4]
            ln = self.r.randrange(lo, hi + 1)
            if not self.to_L and self.L - P[m] <= 420:
                ln = self.L - P[m]
        if self.L - P[m] < 24 or ln > self.L - P[m]:
            return None
        mod4 = None
        if self.kind == "big_steps":
            where = self.n % 6
            fr = first_resident(P[m])
            if where == 4:
                s = self.source(ctx, fr - 500, fr - 8, ln)
            elif where == 5:
                s = self.source(ctx, 32512, 32768, ln)
            else:
                mod4 = self.n % 4
                s = self.source(ctx, 16, BIG_FAR_SRC - 420, ln, mod4)
        else:
            s = self.source(ctx, 1, ctx.p, ln)
        if s is None:
            return None
        if not self.copy(ctx, P[m], s, ln):
            self.undo(ctx)
            return None
        if P[m] + ln < self.L and ctx.bp[P[m] + ln] == ctx.bp[s + ln]:
            self.put(ctx, P[m] + ln, ctx.bp[s + ln] ^ 0x55)
        if not self.wr:
            return None
        if P[m] + ln == self.L:
            self.to_L = True
        self.n += 1
        self.fails = 0
        return self.done()

    def ls_plan(self, ctx):
        """Where lane-space rounds begin (window q0 = p - 1, everything from p + 1 on unread): a
        match from lane 6 to lane E, after which the rounds end at lane 62, the window moves and
        one full round leaves skip = s0 in 61..64 for the W round; then a plant at the probe
        positions pos(s) = end + skipsum(s) that follow if all of them miss."""
        dmax = ctx.dmax
        s0 = 61 if self.kind == "hits" else 61 + self.cycle % 4
        E = 63 - (s0 - 32 - 2 * dmax) - dmax
        q0, ln = ctx.q0, E - 6
        if self.L - ctx.p < 130:
            return None
        s = self.source(ctx, 1, ctx.p, ln)
        if s is None:
            return None
        pf = q0 + 6
        ok = self.copy(ctx, pf, s, ln)
        if ok and ctx.bp[pf + ln] == ctx.bp[s + ln]:
            ok = self.put(ctx, pf + ln, ctx.bp[s + ln] ^ 0x55)
        if not ok:
            self.undo(ctx)
            return None
        pe = pf + ln
        free, ctx.free = ctx.free, pe + 1

        def pos(sv):
            return pe + skipsum(sv)
        if self.kind == "hits":
            k = self.cycle % 3
            n = self.r.randrange(4, 40)
            s2 = self.source(ctx, 1, ctx.p, n)
            if s2 is not None and self.copy(ctx, pos(61 + k), s2, n):
                if ctx.bp[pos(61 + k) + n] == ctx.bp[s2 + n]:
                    self.put(ctx, pos(61 + k) + n, ctx.bp[s2 + n] ^ 0x55)
            self.hold = pos(61 + k)
            self.n += 1
        else:
            mode = "abbc"[(self.cycle // 4) % 4]
            k = 1 + (self.cycle // 16) % 3
            v = self.r.randrange(256)
            if mode == "a":     # a run across lanes k - 1 and k of the first W round
                sv, run = s0 + k, 5 + self.cycle % 3
            else:               # the first round whose lane k follows a step of 2
                ri = 0
                while s0 + 4 * ri + k - 1 < 64:
                    ri += 1
                sv, run = s0 + 4 * ri + k, 5 if mode == "b" else 6 + self.cycle % 2
            a0 = pos(sv - 1)
            self.put(ctx, a0 - 1, v ^ 0xFF)
            for i in range(run):
                self.put(ctx, a0 + i, v)
            self.put(ctx, a0 + run, v ^ 0xFF)
            if mode == "b":     # the run's word again two probes on: the slot's owner shows in the offset
                for i in range(4):
                    self.put(ctx, pos(sv + 2) + i, v)
                self.put(ctx, pos(sv + 2) + 4, v ^ 0xFF)
            self.hold = pos(sv + 3)
        ctx.free = free
        self.cycle += 1
        return self.done()


@functools.lru_cache(maxsize=None)
def unit(name: str, L: int, big: bool, u: int):
    """One unit built against the model, as (bytes, tokens, size, trace); it replays to the same."""
    seed = (SEEDS[name], L, u)
    bp = bytearray(np.random.default_rng(seed).integers(0, 256, L, dtype=np.uint8).tobytes()) + bytes(4)
    hook = None if name == "tails" else Planter(name, L, big, seed)
    toks, size, tr = _run(bp, L, big, None, hook)
    b = bytes(bp[:L])
    again = w_model(b, big)
    assert again[0] == toks and again[1] == size and again[2] == tr, (name, L, u)
    return b, toks, size, tr


@functools.lru_cache(maxsize=None)
def make(name: str, L: int, big: bool, units: int) -> np.ndarray:
    a = np.frombuffer(b"".join(unit(name, L, big, u)[0] for u in range(units)), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(name: str, L: int, big: bool, units: int):
    """The oracle's streams of the units of make()."""
    out, offs = oracle.compress_streams(make(name, L, big, units), L)
    return out.tobytes(), offs.copy()


def traces(name: str, L: int, big: bool, units: int):
    """Per unit the trace; the model's tokens against probe_unit's, its size against the oracle's."""
    _, offs = want(name, L, big, units)
    res = []
    for u in range(units):
        b, toks, size, tr = unit(name, L, big, u)
        hdr = 1 + (L >= 128) + (L >= 16384)
        assert hdr + size == int(offs[u + 1]) - int(offs[u]), (name, L, u)
        serial = probe_unit(b)
        assert toks == serial[0] and size == serial[1], (name, L, u)
        res.append(tr)
    return res


def total(trs):
    t = collections.Counter()
    for tr in trs:
        for key, v in tr.items():
            if key == "max_pend_w":
                t[key] = max(t.get(key, -1), v)
            else:
                t[key] += v
    return t


def show(label, t):
    print(label, " ".join("%s=%d" % kv for kv in sorted(t.items())))


def mutant_differs(name: str, L: int, big: bool, units: int, drop: str):
    """Per unit: does the model with one rule changed give other tokens than the serial ones?"""
    res = []
    for u in range(units):
        b, toks, _, _ = unit(name, L, big, u)
        res.append(w_model(b, big, drop)[0] != toks)
    return res


@functools.lru_cache(maxsize=None)
def tail_input(L: int) -> np.ndarray:
    return make("tails", L, False, 4)


def test_inputs_have_their_properties():
    """No GPU.  Every unit of every input: the model's tokens are probe_unit's serial tokens and its
    size the oracle's (traces()), and the unit replays to the trace it was built with (unit()).
    Then the edges, per input and unit size.  The bounds are conditions on the generators: 20 of
    each equal-word class and 3 of each different-word class at 32,768 and 65,536 bytes per unit
    (four units), 1 of every other edge where it can occur."""
    maxpend = -1
    for big, L, units in [(False, c, units_of(c)) for c in K1R_CHUNKS] + [(True, BLOCK, 4), (True, SHORT, 4),
                                                                         (True, SMALLEST64, 4)]:
        names = ["conf_same"] if L == SMALLEST64 else (BIG_INPUTS if big else K1R_INPUTS)
        full = L >= 32768
        for name in names:
            t = total(traces(name, L, big, units))
            show("%s L=%d big=%d:" % (name, L, big), t)
            maxpend = max(maxpend, t["max_pend_w"])
            assert t["w_flush"] == 0 and t["max_pend_w"] < 64, (name, L)
            if name == "conf_same":
                for rule, d in CLASSES:
                    assert t["same_%s%d" % (rule, d)] >= (20 if full else 1), (name, L, rule, d)
                assert t["hit0"] >= (100 if full else 10), (name, L)
                if L >= 1000:
                    assert min(t["step_s2"], t["step_s3"], t["step_s4_8"]) >= 1, (name, L)
                if full:
                    assert t["step_s9_16"] >= 1, (name, L)
            elif name == "conf_diff":
                for rule, d in CLASSES:
                    assert t["diff_%s%d" % (rule, d)] >= (3 if full else 1), (name, L, rule, d)
                if L >= 1000:
                    assert t["tagcoll0_after_conf"] >= 1, (name, L)
            elif name == "dup":
                for s in (61, 62, 63, 64):
                    assert t["start%d" % s] >= 1, (name, L, s)
                assert t["reuse_inloop_window"] >= 1 and t["reuse_ls_window"] >= 1, (name, L)
                assert t["dup_pass"] >= 1 and t["same_ah1_step2"] >= 1 and t["same_hh1"] >= 1, (name, L)
                assert t["step_s1"] >= 1, (name, L)
            elif name == "hits":
                for k in range(W):
                    assert t["hit%d" % k] >= 1, (name, L, k)
                    if L >= 1000:
                        assert t["hit%d_s2" % k] >= 1, (name, L, k)
                    if L >= 2048:
                        assert min(t["hit%d_s3" % k], t["hit%d_s4_8" % k]) >= 1, (name, L, k)
                    if full:  # (a hit at step 17 or more needs 4,352 bytes of misses: lanes 0-2 see the window's edge)
                        assert t["hit%d_s9_16" % k] >= 1, (name, L, k)
                    if full and k < 3:  # (lane 3 of a W round never has a step of 1)
                        assert t["hit%d_s1" % k] >= 1, (name, L, k)
                if full:
                    assert sum(t["hit%d_s17_45" % k] for k in range(W)) >= 1, (name, L)
                    assert t["len_to_L"] >= 1, (name, L)
                if L >= 2048:
                    assert min(t["len_4_11"], t["len_12_63"], t["len_64_139"], t["len_259"]) >= 1, (name, L)
            elif name == "tails":
                if full:
                    assert t["step_s17_45"] >= 1 and t["all_miss"] >= 1 and t["win_move"] >= 1, (name, L)
            else:  # big_steps
                assert t["step_s52"] >= 1 and t["winedge1"] >= 1 and t["ring_adv_w"] >= 20, (name, L)
                assert t["wfar"] >= 8 and min(t["wfar_c%d" % r] for r in range(4)) >= 1, (name, L)
                assert t["wedge"] >= 1 and t["wwrap"] >= 1, (name, L)
        # over the inputs of one unit size: every stop reason and both window paths
        t = total(tr for name in names for tr in traces(name, L, big, units))
        if len(names) > 1:
            reasons = ["all_miss", "win_reuse", "win_move", "reuse_ls_window"]
            reasons += ["hit%d" % k for k in range(W)] + ["conf%d" % k for k in range(1, W)]
            if L >= 1000:
                reasons += ["tagcoll%d" % k for k in range(W)] + ["winedge%d" % k for k in (2, 3)]
            if L >= 4096:
                reasons += ["winedge1"]
            for key in reasons:
                assert t[key] >= 1, (L, key)
    # the block end at lanes 1-3, and where sk >> 5 changes at the cut
    skcross = 0
    for base in TAIL_BASES:
        t = total(tr for i in range(TAIL_COUNT) for tr in traces("tails", base + i, False, 4))
        show("tails %d..%d:" % (base, base + TAIL_COUNT - 1), t)
        maxpend = max(maxpend, t["max_pend_w"])
        # (at 32,7xx bytes the step is 45: lanes 2 and 3 lie past the window's edge before the block's end)
        for k in ((1, 2, 3) if base < 4096 else (1,)):
            assert t["blockend%d" % k] >= 1, (base, k)
        skcross += t["blockend_skcross"]
    assert skcross >= 1
    print("largest pend at a W-round put_token:", maxpend)
    assert maxpend < 64

    # each rule can be seen: the model with one rule changed gives other tokens
    for L, big in ((32768, False), (BLOCK, True)):
        for drop in ("hh", "ha", "ah"):
            d = mutant_differs("conf_same", L, big, 4, drop)
            print("mutant", drop, "L", L, "conf_same units that differ", d)
            assert all(d), (drop, L)
            if not big:  # (the rules are the same code for both kernels)
                e = mutant_differs("conf_diff", L, big, 4, drop)
                print("mutant", drop, "L", L, "conf_diff units that differ", e)
                assert any(e), (drop, L)
        for drop in ("ah", "nd0"):
            d = mutant_differs("dup", L, big, 4, drop)
            print("mutant", drop, "L", L, "dup units that differ", d)
            assert all(d), (drop, L)
        # notdup forced to all-ones only adds false conflicts: the same tokens in more rounds
        for u in range(4):
            b, toks, size, tr = unit("dup", L, big, u)
            mt, ms, mtr = w_model(b, big, "nd1")
            assert mt == toks and ms == size and mtr["wround"] > tr["wround"], (L, u)

    # the oracle decodes what it encoded
    for name in K1R_INPUTS:
        for chunk in K1R_CHUNKS:
            a = make(name, chunk, False, units_of(chunk))
            out, offs = want(name, chunk, False, units_of(chunk))
            back = oracle.decompress_streams(np.frombuffer(out, dtype=np.uint8), offs, a.size, chunk)
            assert np.array_equal(back, a), (name, chunk)


def to_dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def check_streams(codec, a: np.ndarray, chunk: int, out: bytes, want_offs: np.ndarray):
    comp, offs = codec.compress_tensor(to_dev(a), chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, a.size, chunk=chunk, layout=snappy_amd.STREAMS)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", K1R_CHUNKS)
@pytest.mark.parametrize("name", K1R_INPUTS)
def test_k1r_wprobe(codec, name, chunk):
    units = units_of(chunk)
    check_streams(codec, make(name, chunk, False, units), chunk, *want(name, chunk, False, units))


@pytest.mark.gpu
@pytest.mark.parametrize("base", TAIL_BASES)
def test_k1r_tails(codec, base):
    """One launch per unit length, four noise units each: the last rounds meet the block end at every lane."""
    for L in range(base, base + TAIL_COUNT):
        check_streams(codec, tail_input(L), L, *want("tails", L, False, 4))


@functools.lru_cache(maxsize=None)
def big_want(name: str, layout: str, chunk: int, n: int, L: int):
    a = make(name, L, True, 4)[:n]
    if layout == "single":
        return oracle.compress(a.tobytes()), None
    out, offs = oracle.compress_streams(a, chunk)
    return out.tobytes(), offs.copy()


@pytest.mark.gpu
@pytest.mark.parametrize("layout,chunk,n,L", BIG_SHAPES)
@pytest.mark.parametrize("name", BIG_INPUTS)
def test_k1r64_wprobe(codec, name, layout, chunk, n, L):
    a = make(name, L, True, 4)[:n]
    out, want_offs = big_want(name, layout, chunk, n, L)
    if layout == "streams":
        check_streams(codec, a, chunk, out, want_offs)
        return
    comp, offs = codec.compress_tensor(to_dev(a), chunk=chunk, layout=snappy_amd.SINGLE)
    assert comp.cpu().numpy().tobytes() == out
    back = codec.decompress_tensor(comp, offs, n, chunk=chunk, layout=snappy_amd.SINGLE)
    assert np.array_equal(back.cpu().numpy(), a)


@pytest.mark.gpu
def test_k1r64_smallest_unit(codec):
    check_streams(codec, make("conf_same", SMALLEST64, True, 4), SMALLEST64, *want("conf_same", SMALLEST64, True, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("s_in", range(4))
@pytest.mark.parametrize("L,big", [(32768, False), (BLOCK, True)])
def test_one_unit_any_alignment(codec, L, big, s_in):
    """One conf_same unit whose first byte sits s_in bytes past a dword boundary."""
    import torch
    a = make("conf_same", L, big, 4)[:L]
    out, offs_want = want("conf_same", L, big, 4)
    out = out[:int(offs_want[1])]
    cap = codec.max_output(L, L, snappy_amd.STREAMS)
    pad = 64
    xin = torch.zeros(pad + L + pad, dtype=torch.uint8, device="cuda")
    xin[pad + s_in:pad + s_in + L] = to_dev(a)
    buf = torch.full((pad + cap + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = torch.empty(2, dtype=torch.int64, device="cuda")
    back = torch.full((L + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    codec._bind_stream()  # torch's stream: the fills and copies above are ordered before the kernels
    length = codec.compress_ptr(xin.data_ptr() + pad + s_in, L, L, snappy_amd.STREAMS, buf.data_ptr() + pad,
                                offs.data_ptr())
    codec.decompress_ptr(buf.data_ptr() + pad, offs.data_ptr(), L, L, snappy_amd.STREAMS, back.data_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert length == len(out) and got[pad:pad + length].tobytes() == out, (L, s_in)
    assert (got[:pad] == 0xA5).all() and (got[pad + cap:] == 0xA5).all(), (L, s_in)
    assert np.array_equal(back.cpu().numpy()[:L], a), (L, s_in)
