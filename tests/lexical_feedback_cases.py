"""Lexical pseudo-relevance feedback ('Lexical feedback'): the float64 restatement of its arithmetic and the case builders of
tests/test_lexical_feedback_cpu.py and tests/test_gpu_lexical_feedback.py.

Python floats and NumPy float64 scalars are IEEE doubles and every operation below is rounded once, as the kernels' are
(-ffp-contract=off).  The loops are scalar in the direction of the ADDS: a term's (a document's) additions are made one after the other,
in slot (entry) order; only independent accumulators are updated together."""
import numpy as np

E = 4096                 # fz_lexical_feedback_max_entries()
FB_THREADS = 1024        # the feedback kernel's workgroup
FB_SLOTS = 256           # slots it resolves at a time
FB_DEPTH = 3             # rows whose first entries are in flight together
CUT = 1                  # flag bit 0


# ---- a host index: what the walks read ---------------------------------------------------------------------------------------------------
def host_index(model):
    """{N, V, toff, pdoc, val}: val[p] = the model's weight of posting p, exactly what its walk adds (pval, or float64(tf) * idf)."""
    toff, pdoc = model._toff_host, model._pdoc_host
    if model.lexical_mode() == "pv":
        val = model.lexical_tables()[0].cpu().numpy()
    else:
        val = model._ptf_host.astype(np.float64) * np.repeat(model.idf_host, np.diff(toff))
    return dict(N=model.corpus_size, V=len(toff) - 1, toff=toff, pdoc=pdoc, val=val)


def forward_rows(ix):
    """The document-major rows (foff [N + 1], fterm, fval): terms ascending inside a document."""
    term = np.repeat(np.arange(ix["V"], dtype=np.int32), np.diff(ix["toff"]))
    order = np.argsort(ix["pdoc"], kind="stable")
    foff = np.zeros(ix["N"] + 1, dtype=np.int64)
    np.cumsum(np.bincount(ix["pdoc"], minlength=ix["N"]), out=foff[1:])
    return foff, term[order], ix["val"][order]


def host_forward(model):
    """Give a model built on the CPU its forward index (ops.forward_index sorts on the device): the same three arrays from NumPy."""
    import torch
    from fusion_amd import ops
    toff, pdoc, N = model._toff_host, model._pdoc_host, model.corpus_size
    term = np.repeat(np.arange(len(toff) - 1, dtype=np.int32), np.diff(toff))
    order = np.argsort(pdoc, kind="stable")
    foff = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(pdoc, minlength=N), out=foff[1:])
    model.forward = ops.ForwardIndex(torch.from_numpy(foff), torch.from_numpy(term[order].copy()), torch.from_numpy(order.astype(np.int32)), N, len(toff) - 1)
    return model


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def feedback_ref(foff, fterm, fval, N, id_base, queries, fb_ids, fb_len, coef, alpha, beta, m, cap=E):
    """queries: a list of term-id lists.  -> ([(terms, weights)] per query, flags)."""
    out, flags = [], 0
    F = fb_ids.shape[1]
    for q, qt in enumerate(queries):
        w, total = {}, 0
        flen = (F if fb_len is None else min(max(int(fb_len[q]), 0), F)) if N > 0 else 0
        for r in range(flen):
            d = int(fb_ids[q, r]) - id_base
            if not 0 <= d < N:
                continue
            n = int(foff[d + 1] - foff[d])
            if total + n > cap:
                flags |= CUT
                break
            total += n
            c = float(coef[q, r])
            for e in range(int(foff[d]), int(foff[d + 1])):
                t = int(fterm[e])
                if t >= 0:
                    w[t] = w.get(t, 0.0) + c * float(fval[e])
        own = set(qt)
        cand = sorted(((-x, t) for t, x in w.items() if x > 0 and t not in own))
        sel = cand[:min(m, len(cand))]
        terms, weights = list(qt), [float(alpha)] * len(qt)
        if sel:
            wmax = -sel[0][0]
            for nx, t in sel:
                terms.append(t)
                weights.append(float(beta) * ((-nx) / wmax))
        out.append((terms, weights))
    return out, flags


def plane_ref(ix, entries):
    """[Q, N] float64: per query the chain over its (term, weight) entries of acc = acc + weight * val; a term's postings are distinct
    documents, so one entry updates independent accumulators."""
    out = np.zeros((len(entries), ix["N"]), dtype=np.float64)
    for q, (terms, weights) in enumerate(entries):
        acc = out[q]
        for t, x in zip(terms, weights):
            if t < 0:
                continue
            lo, hi = ix["toff"][t], ix["toff"][t + 1]
            docs = ix["pdoc"][lo:hi]
            acc[docs] = acc[docs] + np.float64(x) * ix["val"][lo:hi]
    return out


def topk_ref(plane, k, id_base=0):
    """(ids [Q, k], scores [Q, k]) of the stable descending ranking, ties to the ascending id (-0.0 == +0.0)."""
    order = np.argsort(-plane, axis=1, kind="stable")[:, :k]
    return order + id_base, np.take_along_axis(plane, order, 1)


def uniform_coef(lens, F):
    """feedback.coefficients(.., beta = 1, 'uniform'): float32(1 / fb_len) in the listed slots."""
    coef = np.zeros((len(lens), F), dtype=np.float32)
    for q, n in enumerate(lens):
        coef[q, :n] = np.float32(1.0 / max(n, 1))
    return coef


def search_feedback_ref(ix, queries, k, fb_docs, fb_terms, alpha, beta, id_base=0):
    """The three steps by the restatement alone: first search, feedback (uniform coefficients), second search.
    -> (first ids, second ids, second scores, expanded entries)."""
    ones = [(qt, [1.0] * len(qt)) for qt in queries]
    first, _ = topk_ref(plane_ref(ix, ones), k, id_base)
    F = min(fb_docs, first.shape[1])
    lens = np.full(len(queries), F, dtype=np.int32)
    foff, fterm, fval = forward_rows(ix)
    exp, _ = feedback_ref(foff, fterm, fval, ix["N"], id_base, queries, first[:, :F], lens, uniform_coef(lens, F), alpha, beta, fb_terms)
    ids, sc = topk_ref(plane_ref(ix, exp), k, id_base)
    return first, ids, sc, exp


# ---- case builders -----------------------------------------------------------------------------------------------------------------------
def synthetic_text(rng, n_docs, lo, hi, vocab_size=3000, prefix="w"):
    vocab = np.array([f"{prefix}{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    return [" ".join(w) for w in np.split(words, np.cumsum(sizes)[:-1])]


def random_rows(rng, lens, V, signed=False):
    """Rows of the given lengths with unique terms of [0, V): (foff, fterm int32, fval float64)."""
    foff = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=foff[1:])
    fterm = np.concatenate([rng.choice(V, size=int(n), replace=False) for n in lens] or [np.zeros(0)]).astype(np.int32)
    fval = rng.uniform(0.1, 3.0, fterm.size)
    if signed:
        fval *= rng.choice([-1.0, 1.0], fterm.size)
    return foff, fterm, fval


def csr(lists, dtype=np.int32):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.array([t for x in lists for t in x] or [0], dtype=dtype)


PLANTED_SEEDS = (3, 5, 8)
PLANTED_K = 30


def planted_cluster(seed):
    """A corpus of 400 background documents and a cluster of 40 that share a vocabulary ('c*' words) the query does not contain; only a
    quarter of the cluster holds the query's topic word.  -> (documents, queries, the cluster's document positions)."""
    rng = np.random.default_rng(seed)
    docs = synthetic_text(rng, 400, 8, 20, vocab_size=300)
    cwords = [f"c{i}" for i in range(8)]
    cluster = []
    for j in range(40):
        body = list(rng.choice(cwords, size=5, replace=False)) + synthetic_text(rng, 1, 3, 6, vocab_size=300)[0].split()
        if j % 4 == 0:
            body.append("topic")
        rng.shuffle(body)
        cluster.append(" ".join(body))
    for j in range(0, 400, 57):                                    # the topic word also strays into the background
        docs[j] += " topic"
    at = sorted(rng.choice(440, size=40, replace=False).tolist())
    out, ci, di = [], iter(cluster), iter(docs)
    for i in range(440):
        out.append(next(ci) if i in set(at) else next(di))
    return out, ["topic w3", "topic"], np.array(at)


def cluster_recall(ids, cluster):
    return [len(set(row.tolist()) & set(cluster.tolist())) / len(cluster) for row in ids]
