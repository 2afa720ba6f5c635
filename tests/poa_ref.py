"""A restatement of the poa contract in Python: spoa's SisdAlignmentEngine for kNW (initialize, the linear,
affine and convex fills and their three walks) and Graph (add_alignment, add_sequence, add_edge,
topological_sort, traverse_heaviest_bundle, branch_completion, generate_consensus()). The fill is written cell
by cell and column by column as the reference writes it, on Python lists, so it is slow and meant for small items.

It counts the labels of LABELS into a dict. A guard raises Guard where the reference would read outside its
matrices or go on with stale indices.

Three labels need a word, because a global alignment cannot meet them in their first sense:
- up_q_open has the minimum 0: no comparison of the convex walk can tell an opening priced at q. Its own test
  H == H[pred] + q is never the first to hold, since H >= F >= H[pred] + g > H[pred] + q. Where the extend-up loop
  stops, F matches no F[pred] + e and O no O[pred] + c, so F = max H[pred] + g and O = max H[pred] + q over the same
  predecessors: the first one with O == H[pred] + q also has F == H[pred] + g, which the loop tests first. The
  label counts both places all the same, and the recorder found none in them.
- head_run, tail_run: every position of the sequence has a pair under kNW, so add_alignment's add_sequence calls
  for the bases before the first and after the last aligned position never make a node. The labels count an
  alignment that begins, or ends, with pairs (-1, position): new source, or sink, nodes."""
import numpy as np

NEG_INF = -(1 << 31) + 1024
LINEAR, AFFINE, CONVEX = 0, 1, 2

LABELS = ("row_pred_ge2", "row_pred_ge4", "diag_pred_ge1", "up_f_ext", "up_o_ext", "up_g_open", "up_q_open",
          "left_e_ext", "left_q_ext", "left_open", "ext_up_ge2_nonfirst", "ext_left_ge2", "mismatch_join",
          "mismatch_new", "head_run", "tail_run", "branch_completion", "bundle_tie_le")
MINIMA = {k: 0 if k == "up_q_open" else 1 for k in LABELS}


class Guard(Exception):
    pass


def new_counts():
    return {k: 0 for k in LABELS}


def subtype(p):
    """(subtype, (m, n, g, e, q, c) as the engine holds them): createAlignmentEngine's rule."""
    m, n, g, e, q, c = (int(x) for x in p)
    if g > 0 or q > 0:
        raise ValueError("gap opening penalty must be non-positive!")
    if e > 0 or c > 0:
        raise ValueError("gap extension penalty must be non-positive!")
    sub = LINEAR if g >= e else (AFFINE if (g <= q or e >= c) else CONVEX)
    if sub == LINEAR:
        e = g
    elif sub == AFFINE:
        q, c = g, e
    return sub, (m, n, g, e, q, c)


class View:
    """A graph in rank order, as gb_poa_align takes it."""

    def __init__(self, base, id, out, in_end, pred):
        self.base, self.id, self.out = [int(x) for x in base], [int(x) for x in id], [int(x) for x in out]
        self.in_end, self.pred = [int(x) for x in in_end], [int(x) for x in pred]
        self.n = len(self.base)

    def preds(self, r):
        """Row indices (rank + 1) of the predecessors of rank r; [0] for a node without in-edges."""
        b = self.in_end[r - 1] if r else 0
        ps = [p + 1 for p in self.pred[b:self.in_end[r]]]
        return ps if ps else [0]

    def edges(self, r):
        b = self.in_end[r - 1] if r else 0
        return [p + 1 for p in self.pred[b:self.in_end[r]]]


def fill(p, view, seq):
    """The matrices after the fill, as lists of rows, and (max_i, score): (H, F, E, O, Q), None where the subtype
    has none."""
    sub, (m, n, g, e, q, c) = subtype(p)
    seq = [int(x) for x in bytes(seq)]
    L, N = len(seq), view.n
    W = L + 1
    H = [[0] * W for _ in range(N + 1)]
    F = E = O = Q = None
    if sub >= AFFINE:
        F, E = [[0] * W for _ in range(N + 1)], [[0] * W for _ in range(N + 1)]
    if sub == CONVEX:
        O, Q = [[0] * W for _ in range(N + 1)], [[0] * W for _ in range(N + 1)]
    # initialize
    if sub == CONVEX:
        for j in range(1, W):
            O[0][j], Q[0][j] = NEG_INF, q + (j - 1) * c
        for i in range(1, N + 1):
            ed = view.edges(i - 1)
            pen = q - c if not ed else NEG_INF
            for pi in ed:
                pen = max(pen, O[pi][0])
            O[i][0], Q[i][0] = pen + c, NEG_INF
    if sub >= AFFINE:
        for j in range(1, W):
            F[0][j], E[0][j] = NEG_INF, g + (j - 1) * e
        for i in range(1, N + 1):
            ed = view.edges(i - 1)
            pen = g - e if not ed else NEG_INF
            for pi in ed:
                pen = max(pen, F[pi][0])
            F[i][0], E[i][0] = pen + e, NEG_INF
    if sub == CONVEX:
        for j in range(1, W):
            H[0][j] = max(Q[0][j], E[0][j])
        for i in range(1, N + 1):
            H[i][0] = max(O[i][0], F[i][0])
    elif sub == AFFINE:
        for j in range(1, W):
            H[0][j] = E[0][j]
        for i in range(1, N + 1):
            H[i][0] = F[i][0]
    else:
        for j in range(1, W):
            H[0][j] = j * g
        for i in range(1, N + 1):
            ed = view.edges(i - 1)
            pen = 0 if not ed else NEG_INF
            for pi in ed:
                pen = max(pen, H[pi][0])
            H[i][0] = pen + g
    # rows in rank order
    best, best_i = NEG_INF, -1
    for r in range(N):
        i = r + 1
        prof = [0] + [m if view.base[r] == s else n for s in seq]
        ps = view.preds(r)
        Hr = H[i]
        Hp = H[ps[0]]
        if sub == LINEAR:
            for j in range(1, W):
                Hr[j] = max(Hp[j - 1] + prof[j], Hp[j] + g)
            for pi in ps[1:]:
                Hp = H[pi]
                for j in range(1, W):
                    Hr[j] = max(Hp[j - 1] + prof[j], max(Hr[j], Hp[j] + g))
            for j in range(1, W):
                Hr[j] = max(Hr[j - 1] + g, Hr[j])
        else:
            Fr, Fp = F[i], F[ps[0]]
            for j in range(1, W):
                Fr[j] = max(Hp[j] + g, Fp[j] + e)
                Hr[j] = Hp[j - 1] + prof[j]
            if sub == CONVEX:
                Or, Op = O[i], O[ps[0]]
                for j in range(1, W):
                    Or[j] = max(Hp[j] + q, Op[j] + c)
            for pi in ps[1:]:
                Hp, Fp = H[pi], F[pi]
                for j in range(1, W):
                    Fr[j] = max(Fr[j], max(Hp[j] + g, Fp[j] + e))
                    Hr[j] = max(Hr[j], Hp[j - 1] + prof[j])
                if sub == CONVEX:
                    Op = O[pi]
                    for j in range(1, W):
                        Or[j] = max(Or[j], max(Hp[j] + q, Op[j] + c))
            Er = E[i]
            if sub == CONVEX:
                Qr = Q[i]
                for j in range(1, W):
                    Er[j] = max(Hr[j - 1] + g, Er[j - 1] + e)
                    Qr[j] = max(Hr[j - 1] + q, Qr[j - 1] + c)
                    Hr[j] = max(Hr[j], max(max(Fr[j], Er[j]), max(Or[j], Qr[j])))
            else:
                for j in range(1, W):
                    Er[j] = max(Hr[j - 1] + g, Er[j - 1] + e)
                    Hr[j] = max(Hr[j], max(Fr[j], Er[j]))
        if not view.out[r] and best < Hr[W - 1]:
            best, best_i = Hr[W - 1], i
    return (H, F, E, O, Q), best_i, best


def align(p, view, seq, counts=None):
    """(pairs as a list of (node id or -1, position or -1), score) of SisdAlignmentEngine::align."""
    if view.n == 0 or len(seq) == 0:
        return [], 0
    cnt = counts if counts is not None else new_counts()
    sub, (m, n, g, e, q, c) = subtype(p)
    (H, F, E, O, Q), max_i, score = fill(p, view, seq)
    seq = [int(x) for x in bytes(seq)]
    for r in range(view.n):
        k = len(view.edges(r))
        cnt["row_pred_ge2"] += k >= 2
        cnt["row_pred_ge4"] += k >= 4
    if max_i < 0:
        raise Guard("no node without out-edges")
    out = []
    i, j, prev_i, prev_j = max_i, len(seq), 0, 0
    bound = view.n + len(seq)
    while not (i == 0 and j == 0):
        h = H[i][j]
        found = ext_left = ext_up = False
        if i != 0 and j != 0:
            mc = m if view.base[i - 1] == seq[j - 1] else n
            for k, pi in enumerate(view.preds(i - 1)):
                if h == H[pi][j - 1] + mc:
                    prev_i, prev_j, found = pi, j - 1, True
                    cnt["diag_pred_ge1"] += k >= 1
                    break
        if not found and i != 0:
            for pi in view.preds(i - 1):
                if sub == LINEAR:
                    hit = h == H[pi][j] + g
                    why = "up_g_open"
                elif sub == AFFINE:
                    ext_up = h == F[pi][j] + e
                    hit = ext_up or h == H[pi][j] + g
                    why = "up_f_ext" if ext_up else "up_g_open"
                else:
                    ext_up = h == F[pi][j] + e
                    why = "up_f_ext"
                    hit = ext_up
                    if not hit:
                        hit, why = h == H[pi][j] + g, "up_g_open"
                    if not hit:
                        ext_up = hit = h == O[pi][j] + c
                        why = "up_o_ext"
                    if not hit:
                        hit, why = h == H[pi][j] + q, "up_q_open"
                if hit:
                    prev_i, prev_j, found = pi, j, True
                    cnt[why] += 1
                    break
        if not found and j != 0:
            if sub == LINEAR:
                hit, why = h == H[i][j - 1] + g, "left_open"
            elif sub == AFFINE:
                ext_left = h == E[i][j - 1] + e
                hit = ext_left or h == H[i][j - 1] + g
                why = "left_e_ext" if ext_left else "left_open"
            else:
                ext_left = h == E[i][j - 1] + e
                hit, why = ext_left, "left_e_ext"
                if not hit:
                    hit, why = h == H[i][j - 1] + g, "left_open"
                if not hit:
                    ext_left = hit = h == Q[i][j - 1] + c
                    why = "left_q_ext"
                if not hit:
                    hit, why = h == H[i][j - 1] + q, "left_open"
            if hit:
                prev_i, prev_j, found = i, j - 1, True
                cnt[why] += 1
        if not found:
            raise Guard(f"cell ({i}, {j}) matches no move")
        out.append((-1 if i == prev_i else view.id[i - 1], -1 if j == prev_j else j - 1))
        i, j = prev_i, prev_j
        if ext_left:
            steps = 0
            while True:
                if j == 0:
                    raise Guard("extend-left at column 0")
                out.append((-1, j - 1))
                j -= 1
                steps += 1
                e_ends = E[i][j] + e != E[i][j + 1]
                if e_ends if sub == AFFINE else (e_ends and Q[i][j] + c != Q[i][j + 1]):
                    break
            cnt["ext_left_ge2"] += steps >= 2
        elif ext_up:
            steps, nonfirst = 0, False
            while True:
                if i == 0:
                    raise Guard("extend-up at row 0")
                prev_i, f = 0, F[i][j]
                ed = view.edges(i - 1)
                if sub == AFFINE:
                    stop = False
                    for k, pi in enumerate(ed):
                        stop = f == H[pi][j] + g
                        if stop or f == F[pi][j] + e:
                            prev_i, nonfirst = pi, nonfirst or k >= 1
                            break
                else:
                    o, stop = O[i][j], True
                    for k, pi in enumerate(ed):
                        if f == F[pi][j] + e or o == O[pi][j] + c:
                            prev_i, stop, nonfirst = pi, False, nonfirst or k >= 1
                            break
                    if stop:
                        for k, pi in enumerate(ed):
                            if f == H[pi][j] + g or o == H[pi][j] + q:
                                prev_i, nonfirst = pi, nonfirst or k >= 1
                                cnt["up_q_open"] += f != H[pi][j] + g
                                break
                out.append((view.id[i - 1], -1))
                i = prev_i
                steps += 1
                if stop or i == 0:
                    break
            cnt["ext_up_ge2_nonfirst"] += steps >= 2 and nonfirst
        if len(out) > bound:
            raise Guard("the walk passed nodes + bases")
    out.reverse()
    return out, score


def f32_sum_u32(prev, w):
    """uint32(float(prev) + float(w)) in single precision, as the reference's add_edge arguments."""
    return int(np.uint32(np.float32(prev) + np.float32(np.uint32(w))))


class Graph:
    def __init__(self):
        self.base, self.ins, self.outs, self.aligned = [], [], [], []  # per node; ins / outs hold edge indices
        self.edges = []  # [begin, end, weight]
        self.rank_to_node = []
        self.num_sequences = 0

    def add_node(self, b):
        self.base.append(int(b)), self.ins.append([]), self.outs.append([]), self.aligned.append([])
        return len(self.base) - 1

    def add_edge(self, b, e, w):
        w &= 0xffffffff
        for k in self.outs[b]:
            if self.edges[k][1] == e:
                self.edges[k][2] += w
                return
        self.edges.append([b, e, w])
        self.outs[b].append(len(self.edges) - 1), self.ins[e].append(len(self.edges) - 1)

    def add_sequence(self, seq, wt, begin, end):
        if begin == end:
            return -1
        first = self.add_node(seq[begin])
        for i in range(begin + 1, end):
            nid = self.add_node(seq[i])
            self.add_edge(nid - 1, nid, int(wt[i - 1]) + int(wt[i]))
        return first

    def add_alignment(self, pairs, seq, wt=None, counts=None):
        cnt = counts if counts is not None else new_counts()
        seq = bytes(seq)
        if len(seq) == 0:
            return
        wt = [1] * len(seq) if wt is None else [int(x) for x in wt]
        if not pairs:
            self.add_sequence(seq, wt, 0, len(seq))
            self.num_sequences += 1
            self.topological_sort()
            return
        valid = [b for _, b in pairs if b != -1]
        before = len(self.base)
        self.add_sequence(seq, wt, 0, valid[0])
        head = -1 if before == len(self.base) else len(self.base) - 1
        tail = self.add_sequence(seq, wt, valid[-1] + 1, len(seq))
        if head != -1 or tail != -1:
            raise Guard("a base without a pair under kNW")
        cnt["head_run"] += pairs[0][0] == -1
        cnt["tail_run"] += pairs[-1][0] == -1
        node, prev_weight = -1, (0 if head == -1 else wt[valid[0] - 1])
        for at, pos in pairs:
            if pos == -1:
                continue
            letter = seq[pos]
            if at == -1:
                node = self.add_node(letter)
            elif self.base[at] == letter:
                node = at
            else:
                to = -1
                for aid in self.aligned[at]:
                    if self.base[aid] == letter:
                        to = aid
                        break
                if to == -1:
                    node = self.add_node(letter)
                    for aid in list(self.aligned[at]):
                        self.aligned[node].append(aid), self.aligned[aid].append(node)
                    self.aligned[node].append(at), self.aligned[at].append(node)
                    cnt["mismatch_new"] += 1
                else:
                    node = to
                    cnt["mismatch_join"] += 1
            if head != -1:
                self.add_edge(head, node, f32_sum_u32(prev_weight, wt[pos]))
            head, prev_weight = node, wt[pos]
        if tail != -1:
            self.add_edge(head, tail, f32_sum_u32(prev_weight, wt[valid[-1] + 1]))
        self.num_sequences += 1
        self.topological_sort()

    def topological_sort(self):
        n = len(self.base)
        self.rank_to_node = []
        mark, check, stack = [0] * n, [True] * n, []
        for i in range(n):
            if mark[i] != 0:
                continue
            stack.append(i)
            while stack:
                nid, valid = stack[-1], True
                if mark[nid] != 2:
                    for k in self.ins[nid]:
                        b = self.edges[k][0]
                        if mark[b] != 2:
                            stack.append(b)
                            valid = False
                    if check[nid]:
                        for aid in self.aligned[nid]:
                            if mark[aid] != 2:
                                stack.append(aid)
                                check[aid] = False
                                valid = False
                    if valid:
                        mark[nid] = 2
                        if check[nid]:
                            self.rank_to_node.append(nid)
                            self.rank_to_node.extend(self.aligned[nid])
                    else:
                        mark[nid] = 1
                if valid:
                    stack.pop()
        assert len(self.rank_to_node) == n

    def view(self):
        rank = [0] * len(self.base)
        for r, nid in enumerate(self.rank_to_node):
            rank[nid] = r
        base, ids, out, in_end, pred = [], [], [], [], []
        for nid in self.rank_to_node:
            base.append(self.base[nid]), ids.append(nid), out.append(1 if self.outs[nid] else 0)
            pred += [rank[self.edges[k][0]] for k in self.ins[nid]]
            in_end.append(len(pred))
        return View(base, ids, out, in_end, pred)

    def _pick(self, nid, scores, preds, skip, cnt):
        for k in self.ins[nid]:
            b, _, w = self.edges[k]
            if skip and scores[b] == -1:
                continue
            if scores[nid] < w:
                scores[nid], preds[nid] = w, b
            elif scores[nid] == w:
                if preds[nid] == -1:
                    raise Guard("heaviest bundle reads scores[-1]")
                if scores[preds[nid]] <= scores[b]:
                    scores[nid], preds[nid] = w, b
                    cnt["bundle_tie_le"] += 1
        if preds[nid] != -1:
            scores[nid] += scores[preds[nid]]

    def consensus(self, counts=None):
        cnt = counts if counts is not None else new_counts()
        n = len(self.base)
        if n == 0:
            return b""
        preds, scores, best = [-1] * n, [-1] * n, 0
        for nid in self.rank_to_node:
            self._pick(nid, scores, preds, False, cnt)
            if scores[best] < scores[nid]:
                best = nid
        if self.outs[best]:
            rank = [0] * n
            for r, nid in enumerate(self.rank_to_node):
                rank[nid] = r
            while self.outs[best]:
                cnt["branch_completion"] += 1
                node_id = best
                for k in self.outs[node_id]:
                    for o in self.ins[self.edges[k][1]]:
                        if self.edges[o][0] != node_id:
                            scores[self.edges[o][0]] = -1
                max_score, best = 0, 0
                for r in range(rank[node_id] + 1, n):
                    nid = self.rank_to_node[r]
                    scores[nid], preds[nid] = -1, -1
                    self._pick(nid, scores, preds, True, cnt)
                    if max_score < scores[nid]:
                        max_score, best = scores[nid], nid
        out = []
        while preds[best] != -1:
            out.append(self.base[best])
            best = preds[best]
        out.append(self.base[best])
        return bytes(reversed(out))


def rank_checksum(order):
    """A checksum of rank_to_node_id: sum of (rank + 1) * (node id + 1) modulo 2^61 - 1."""
    a = np.asarray(order, np.int64)
    return int(((np.arange(1, len(a) + 1, dtype=object) * (a.astype(object) + 1)).sum()) % ((1 << 61) - 1)) if len(a) else 0


def window(p, reads, weights=None, counts=None, on_alignment=None):
    """The rounds of one window: (consensus, node count, alignments done, cells, rank checksum).
    on_alignment(round, view, seq, pairs, score) is called for every alignment done."""
    G = Graph()
    done = cells = 0
    for k, r in enumerate(reads):
        r = bytes(r)
        pairs = []
        if len(r) and len(G.base):
            v = G.view()
            pairs, score = align(p, v, r, counts)
            done, cells = done + 1, cells + v.n * len(r)
            if on_alignment:
                on_alignment(k, v, r, pairs, score)
        G.add_alignment(pairs, r, None if weights is None else weights[k], counts)
    return G.consensus(counts), len(G.base), done, cells, rank_checksum(G.rank_to_node)
