"""The fused recurrent head of one rollout step (csrc/cma_step.hip) restated in float64 torch from UNFOLDED weights, for
both state-encoder cells: what tests/test_gpu_cma_step_kernels.py and tests/test_gpu_cma_step_lstm.py compare the kernels
with, and what tests/test_cma_step_coverage.py holds the folded form to.  Not a conftest: plain functions, imported by name.

  state = RNN1([dep_in | map_in | prev], h1 * mask)              text = softmax((W_q state + b_q) . text_k * s - 1e8 pad) . txt
  dep'  = softmax((W_tq text + b_tq) . dep_k * s) . dep_v        (map' likewise)
  feats = RNN2(ReLU(W_c [state | text | dep' | map' | prev] + b_c), h2 * mask)

GRU  (csrc/rnn_cell.h; gates r, z, n; state (rows, 2, H) = [h1 | h2]; 3H weight rows):
       r = s(gi_r + gh_r)  z = s(gi_z + gh_z)  n = tanh(gi_n + r gh_n)  h' = (1 - z) n + z (h * mask)
LSTM (gates i, f, g, o; state (rows, 4, H) = [h1 | c1 | h2 | c2]; 4H weight rows):
       c' = s(f) (c * mask) + s(i) tanh(g);  h' = s(o) tanh(c')"""
import torch

EPS = 2.0 ** -24
SMALL = dict(H=64, Hq=32, Ct=16, d_out=16, m_out=32, E=4)
FULL = dict(H=512, Hq=256, Ct=256, d_out=128, m_out=256, E=32)
GATES = {"gru": 3, "lstm": 4}
SLOTS = {"gru": ("h1", "h2"), "lstm": ("h1", "c1", "h2", "c2")}  # the state's slots, in the order the kernels keep them
LAST_POS_FLOORS = 1000  # leaving out a full row's last position must move `text` by this many floors of the bar


def case_seed(rows, L, P, mask0):
    return rows * 10007 + L * 101 + P + mask0


def _rnn64(cell, d, n, x, st, m, H):
    """one masked step of encoder n ("1" / "2") in float64 -> the new slots, in SLOTS order"""
    h = st[0] * m
    gi, gh = x @ d["w_ih" + n].t() + d["b_ih" + n], h @ d["w_hh" + n].t() + d["b_hh" + n]
    if cell == "gru":
        r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        nn = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return ((1.0 - z) * nn + z * h,)
    pre = gi + gh
    i, f, gg, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    ct = f * (st[1] * m) + i * gg
    return o * torch.tanh(ct), ct


def folds64(d):
    """the instruction-only folds in float64 -> (text_k (rows, Hq, L), Mq (rows, H + 1, L), TQb (rows, Hq, L))"""
    rows, Hq, L = d["rows"], d["Hq"], d["L"]
    text_k = torch.einsum("qc,nci->nqi", d["w_k"], d["txt"]) + d["b_k"].view(1, Hq, 1)
    mq = torch.einsum("qh,nqi->nhi", d["w_q"], text_k)
    mq_b = torch.einsum("q,nqi->ni", d["b_q"], text_k).view(rows, 1, L)
    tqb = torch.einsum("qc,nci->nqi", d["w_tq"], d["txt"]) + d["b_tq"].view(1, Hq, 1)
    return text_k, torch.cat([mq, mq_b], 1), tqb


def head64(cell, d, lengths=None, folded=False):
    """The head in float64 on the double operands `d`.  folded: the way the kernels compute it, from [Mq | TQb] (made
    here in float64, NOT rounded): logits = state . Mq + bias row, q2 . k[:, p] = sum_i a_i S[i][p] with S = TQb^T k.
    lengths: in place of d["lengths"].  -> dict of x2 (without prev), feats and the state's slots."""
    rows, L, H, Hq, E, x2w = (d[k] for k in ("rows", "L", "H", "Hq", "E", "x2w"))
    lengths = d["lengths"] if lengths is None else lengths
    m = d["mask"].double().view(rows, 1)
    pad = (torch.arange(L).view(1, L) >= lengths.view(rows, 1)).double()
    st = d["state"]
    n1 = len(SLOTS[cell]) // 2
    s1 = _rnn64(cell, d, "1", d["state_in"], [st[:, k] for k in range(n1)], m, H)
    h1 = s1[0]
    if folded:
        _, mq, tqb = folds64(d)
        a = torch.softmax((torch.einsum("nh,nhi->ni", h1, mq[:, :H]) + mq[:, H] - pad * 1e8) * d["scale"], 1)
        text = torch.einsum("ni,nci->nc", a, d["txt"])
        out = []
        for kv in (d["dkv"], d["mkv"]):
            S = torch.einsum("nci,ncp->nip", tqb, kv[:, :Hq])
            ap = torch.softmax(torch.einsum("ni,nip->np", a, S) * d["scale"], 1)
            out.append(torch.einsum("np,ncp->nc", ap, kv[:, Hq:]))
        dep, mp = out
    else:
        def attn(q, k, v, pad=None):
            lg = torch.einsum("nc,nci->ni", q, k)
            if pad is not None:
                lg = lg - pad * 1e8
            return torch.einsum("ni,nci->nc", torch.softmax(lg * d["scale"], 1), v)

        text_k = torch.einsum("qc,nci->nqi", d["w_k"], d["txt"]) + d["b_k"].view(1, Hq, 1)
        text = attn(h1 @ d["w_q"].t() + d["b_q"], text_k, d["txt"], pad)
        q2 = text @ d["w_tq"].t() + d["b_tq"]
        dep = attn(q2, d["dkv"][:, :Hq], d["dkv"][:, Hq:])
        mp = attn(q2, d["mkv"][:, :Hq], d["mkv"][:, Hq:])
    x2 = torch.cat([h1, text, dep, mp, d["prev"]], 1)
    s2 = _rnn64(cell, d, "2", torch.relu(x2 @ d["w_c"].t() + d["b_c"]), [st[:, n1 + k] for k in range(n1)], m, H)
    ref = dict(x2=x2[:, :x2w - E], feats=s2[0])
    ref.update(zip(SLOTS[cell], s1 + s2))
    return ref


def doubles(c):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}


def make_case(cell, rows, L, P, widths, mask0, seed, lengths=None):
    """Inputs (fp32, CPU) and the float64 restatement of the head from unfolded weights.  lengths (rows ints): in place of
    the drawn ones (a 0 is an empty row: its txt is all zero).  The draw order is that of the LSTM head's first test
    file, whatever the cell, so the LSTM cases see the inputs they always saw."""
    w = widths
    NG = GATES[cell]
    H, Hq, Ct, d_out, m_out, E = (w[k] for k in ("H", "Hq", "Ct", "d_out", "m_out", "E"))
    sin_w, x2w = d_out + m_out + E, H + Ct + d_out + m_out + E
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, k=1.0: torch.randn(*s, generator=g) * k  # noqa: E731
    c = dict(cell=cell, rows=rows, L=L, P=P, sin_w=sin_w, x2w=x2w, **w)
    c["state_in"] = rn(rows, sin_w)
    if cell == "lstm":
        c["state"] = torch.stack([rn(rows, H, k=0.5), rn(rows, H), rn(rows, H, k=0.5), rn(rows, H)], 1)  # h1 c1 h2 c2
    else:
        c["state"] = torch.stack([rn(rows, H, k=0.5), rn(rows, H, k=0.5)], 1)  # h1 h2
    mask = torch.ones(rows, dtype=torch.uint8)
    mask[0] = mask0  # (rows > 1: an episode starts in row 0, whose incoming state is non-zero)
    c["mask"] = mask
    drawn = torch.randint(1, L + 1, (rows,), generator=g).to(torch.int32)
    if L > 1 and rows > 1:
        drawn[1 % rows], drawn[2 % rows] = 1, L  # one row of one token, one of the full axis
    elif L > 1:
        drawn[0] = L
    if lengths is not None:
        assert len(lengths) == rows and all(0 <= int(n) <= L for n in lengths)
        drawn = torch.tensor([int(n) for n in lengths], dtype=torch.int32)
    lengths = c["lengths"] = drawn
    txt = rn(rows, Ct, L)
    txt = txt * (torch.arange(L).view(1, 1, L) < lengths.view(rows, 1, 1))  # the instruction encoder's output is 0 past the end
    c["txt"] = txt
    c["dkv"], c["mkv"] = rn(rows, Hq + d_out, P), rn(rows, Hq + m_out, P)
    c["prev"] = rn(rows, E)
    for n, I in (("1", sin_w), ("2", H)):
        c["w_ih" + n], c["b_ih" + n] = rn(NG * H, I, k=0.7 / I ** 0.5), rn(NG * H, k=0.1)
        c["w_hh" + n], c["b_hh" + n] = rn(NG * H, H, k=0.8 / H ** 0.5), rn(NG * H, k=0.1)
    c["w_q"], c["b_q"] = rn(Hq, H, k=1.0 / H ** 0.5), rn(Hq, k=0.1)
    c["w_k"], c["b_k"] = rn(Hq, Ct, k=1.0 / Ct ** 0.5), rn(Hq, k=0.1)
    c["w_tq"], c["b_tq"] = rn(Hq, Ct, k=1.0 / Ct ** 0.5), rn(Hq, k=0.1)
    c["w_c"], c["b_c"] = rn(H, x2w, k=1.0 / x2w ** 0.5), rn(H, k=0.1)
    c["scale"] = float(1.0 / Hq ** 0.5)  # Hq ** -0.5, in the form the LSTM file always wrote it (the same double)

    d = doubles(c)
    c["ref"] = head64(cell, d)
    if L >= 255:
        # the last position of a full row is live: without it `text` moves by far more than the bar can hide
        full = [r for r in range(rows) if int(lengths[r]) == L]
        assert full, "no row spans the whole instruction axis"
        short = lengths.clone()
        short[full[0]] = L - 1
        o_txt = H
        move = float((head64(cell, d, lengths=short)["x2"] - c["ref"]["x2"])[full[0], o_txt:o_txt + Ct].abs().max())
        floor = 4 * EPS * float(c["ref"]["x2"].abs().max())
        c["last_pos_move"], c["floor"] = move, floor
        assert move >= LAST_POS_FLOORS * floor, (cell, rows, L, P, move, floor)
    # the folds the caller supplies, made in float64 and rounded once: [Mq (H + 1 rows) | TQb (Hq rows)] x L per row
    text_k, mq, tqb = folds64(d)
    c["fold"] = torch.cat([mq, tqb], 1).float()
    c["text_k"] = text_k.float()  # rounded once, for the unfused chain
    return c
