"""Non-finite inputs: the generators, the NaN-aware float64 references and the checkers that tests/test_gpu_nonfinite.py and
tests/test_gpu_scaling.py share (not a test module; tests/test_nonfinite_cpu.py tests it on the CPU).  The contract they hold
the ops to is in include/anyloc_hip.h (Conventions, "Non-finite values"):
  1. containment   a bad unit spoils its own outputs only; every other output has the bits of the clean twin;
  2. propagation   NaN stands where the float64 evaluation of the same formula has NaN;
  3. selections    never pick a NaN: label 0 for an all-NaN row, a NaN-scored database row is never listed, padding is -1;
  4. powers of two are exact.
Everything here runs on the device of its inputs.  The references are built ON the shared ones (``_retrieval_refs``,
``_vlad_refs``, ``_attention_refs``), which propagate NaN by themselves; what is added is the selection rule."""
import torch

import _retrieval_refs as R
import _vlad_refs as V

VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
WHERE = ("first", "last", "col16")
FILL = 0.25          # what the clean twin holds where the bad unit holds its non-finite value: finite, of ordinary size, and below
                     # every maximum the generators' rows have, so that no shared power-of-two scale depends on it


def position(n, where):
    """flat position inside a unit of ``n`` elements: its first element, its last, the one at a 16-column boundary"""
    assert where in WHERE, where
    return {"first": 0, "last": n - 1, "col16": min(16, n - 1)}[where]


def _put(t, unit, where, v):
    out = t.clone()
    sub = out[unit]                                        # basic indexing: a view of ``out``
    idx = torch.unravel_index(torch.tensor(position(sub.numel(), where)), sub.shape) if sub.dim() else ()
    sub[tuple(int(i) for i in idx)] = v
    return out


def plant(t, unit, where, value):
    """-> a copy of ``t`` whose ``unit`` (an index expression of basic indexing: a row, ``(image, token, columns)``, ...) holds
    ``value`` ("nan", "+inf", "-inf", or a number) at position ``where`` of the unit"""
    return _put(t, unit, where, VALUES.get(value, value))


def clean_twin(t, unit, where, fill=FILL):
    """-> the clean twin of ``plant(t, unit, where, ...)``: the same tensor with ``fill`` at that position"""
    return _put(t, unit, where, fill)


def split_view(t):
    """What the two split arithmetics (three bf16 planes, two fp16 planes) hold of ``t``: the residual plane of an infinity
    is inf - inf, so an infinite element is a NaN element there (rule 2, "the same formula")."""
    return torch.where(torch.isinf(t), torch.full_like(t, float("nan")), t)


# ------------------------------------------------------------------------------------------------------------- bits
def bits(t):
    """the bit patterns of a floating tensor, as integers of its width"""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def contained(got, twin, ref, spoiled, rtol=0.0, atol=0.0, tag=""):
    """Rules 1 and 2 on one output.  ``got``: the call with the bad unit; ``twin``: the same call on the clean twin; ``ref``:
    float64 evaluation of the call with the bad unit; ``spoiled``: bool mask (broadcast to the output) of what may differ.
      outside the mask   got has the twin's bits;
      inside             got is NaN exactly where ref is, infinite exactly where ref is (same sign), and elsewhere within
                         atol + rtol * |ref|.
    -> the largest error of the finite spoiled outputs (0.0 when there are none)."""
    assert got.shape == twin.shape == ref.shape and got.dtype == twin.dtype, (tag, got.shape, twin.shape, ref.shape)
    mask = spoiled.to(got.device).expand(got.shape)
    leak = (bits(got) != bits(twin)) & ~mask
    assert not bool(leak.any()), f"{tag}: {int(leak.sum())} clean outputs differ from the twin's bits, first at {leak.nonzero()[0].tolist()}"
    g, r = got.double()[mask], ref.double().to(got.device)[mask]
    missing, extra = torch.isnan(r) & ~torch.isnan(g), torch.isnan(g) & ~torch.isnan(r)
    assert not bool(missing.any()), f"{tag}: {int(missing.sum())} of {g.numel()} spoiled outputs are not NaN where float64 is"
    assert not bool(extra.any()), f"{tag}: {int(extra.sum())} of {g.numel()} spoiled outputs are NaN where float64 is not"
    inf = torch.isinf(r)
    assert bool((g[inf] == r[inf]).all()), f"{tag}: an infinity of float64 is not the same infinity here"
    fin = ~torch.isnan(r) & ~inf
    err = (g[fin] - r[fin]).abs()
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{tag}: {int(mask.sum())} spoiled outputs ({int(torch.isnan(r).sum())} NaN, {int(inf.sum())} inf), largest error of the finite ones {worst:.2e}")
    if torch.is_tensor(atol):                              # one bar per output
        atol = atol.to(got.device).double().expand(got.shape)[mask][fin]
    assert bool((err <= atol + rtol * r[fin].abs()).all()), (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------- labels
def hard_assign_nan(scores):
    """Rule 3 on a float64 score matrix [n, K]: the first largest non-NaN score of a row wins, an all-NaN row gets 0"""
    s = torch.where(torch.isnan(scores), torch.full_like(scores, float("-inf")), scores)
    first = torch.where(s == s.amax(dim=1, keepdim=True), torch.arange(s.shape[1], device=s.device), s.shape[1])
    return first.amin(dim=1)


def assign_scores64(x, centers, euclidean=False):
    """float64 scores of the hard assignment as the kernels form them: x . c / (||c|| + 1e-8) (cosine: the row's own norm
    does not move its arg-max) or 2 x . c - ||c||^2 (euclidean)"""
    xd, cd = x.double(), centers.double()
    if euclidean:
        return 2.0 * xd @ cd.t() - (cd * cd).sum(1)
    return xd @ (cd / (cd.norm(dim=1, keepdim=True) + 1e-8)).t()


def check_labels(labels, scores, tie, tag=""):
    """Rule 3 on the labels of a kernel against the float64 scores [n, K] of the same rows: every label in [0, K); a row whose
    scores are all NaN has label 0; no label points at a NaN score while the row has another; the chosen score is within
    ``tie`` (the arithmetic's error on a score) of the row's best non-NaN one.  -> rows that differ from hard_assign_nan"""
    n, K = scores.shape
    lab = labels.to(scores.device)
    assert lab.shape == (n,) and bool(((lab >= 0) & (lab < K)).all()), f"{tag}: a label outside [0, {K})"
    want = hard_assign_nan(scores)
    nan = torch.isnan(scores)
    dead = nan.all(dim=1)
    assert bool((lab[dead] == 0).all()), f"{tag}: a row of NaN scores without label 0"
    chosen = torch.gather(scores, 1, lab[:, None])[:, 0]
    assert not bool(torch.isnan(chosen[~dead]).any()), f"{tag}: a NaN score won against a number"
    best = torch.gather(scores, 1, want[:, None])[:, 0]
    live = ~dead & torch.isfinite(best)
    tie = torch.as_tensor(tie, dtype=torch.float64, device=scores.device).expand(n)        # (one bar, or one per row)
    assert bool((chosen[live] >= best[live] - tie[live]).all()), (tag, float((best[live] - chosen[live]).max()))
    inf = ~dead & torch.isinf(best)
    assert bool((chosen[inf] == best[inf]).all()), f"{tag}: an infinite score did not compare as a number"
    return int((lab != want).sum())


def hard_vlad_nan(tokens, centers, labels, **kw):
    """``_vlad_refs.hard_vlad_f64`` per image under the given labels (float64 propagates NaN by itself): tokens [n_img, N, D],
    labels [n_img * N] -> [n_img, K * D]"""
    n_img, N, _ = tokens.shape
    return torch.stack([V.hard_vlad_f64(tokens[b], centers, labels[b * N:(b + 1) * N].to(tokens.device), **kw) for b in range(n_img)])


# -------------------------------------------------------------------------------------------------------------- lists
def pad_distance(metric):
    """the distance of a padding entry (index -1): the tail rule of every top-k path"""
    return float("inf") if metric == "l2" else float("-inf")


def flat_search_nan_last(s, k, metric):
    """Rule 3 as a search over a float64 score matrix (larger = better): NaN ranks last and is never listed, neither is -inf;
    ties -> lower index; -> (fp32 distances, int64 indices), padding (pad_distance, -1)"""
    low = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    o = torch.sort(low, dim=1, descending=True, stable=True)
    kk = min(k, s.shape[1])
    d = torch.full((s.shape[0], k), pad_distance(metric), device=s.device)
    i = torch.full((s.shape[0], k), -1, dtype=torch.int64, device=s.device)
    listed = o.values[:, :kk] > float("-inf")
    vals = -o.values[:, :kk] if metric == "l2" else o.values[:, :kk]
    d[:, :kk] = torch.where(listed, vals.float(), d[:, :kk])
    i[:, :kk] = torch.where(listed, o.indices[:, :kk], i[:, :kk])
    return d, i


BIG = 1e300          # stands for an infinity on both sides of check_lists' subtraction


def check_lists_nan(d, i, s, k, metric, tag, index_base=0, scale=1.0, cap=None):
    """Lists (d, i) against a float64 score matrix that may hold NaN and infinities (rule 3), through
    ``_retrieval_refs.check_lists``:
      every index is -1 or inside [index_base, index_base + ndb);
      no listed row has a NaN score; a query without any listable row has the padding list, distances included;
      every other query has at least k listable rows here, and its list passes check_lists against the scores with NaN
      ranked last (infinities compare as numbers).
    -> the number of entries check_lists excused as near-ties."""
    ndb = s.shape[1]
    i = i.to(s.device)
    d = d.to(s.device)
    assert bool(((i == -1) | ((i >= index_base) & (i < index_base + ndb))).all()), f"{tag}: an index outside the database"
    loc = torch.where(i >= 0, i - index_base, i)
    listable = ~torch.isnan(s) & (s > float("-inf"))
    got_nan = torch.gather(torch.isnan(s), 1, loc.clamp_min(0)) & (loc >= 0)
    assert not bool(got_nan.any()), f"{tag}: {int(got_nan.sum())} listed rows have a NaN score, first at {got_nan.nonzero()[0].tolist()}"
    n_ok = listable.sum(dim=1)
    empty = n_ok == 0
    assert bool((loc[empty] == -1).all()), f"{tag}: a query without a listable row lists one"
    assert bool((d[empty] == pad_distance(metric)).all()), f"{tag}: padding distances are not {pad_distance(metric)}"
    full = n_ok >= min(k, ndb)
    assert bool((full | empty).all()), f"{tag}: the checker serves queries with no listable row or with at least k"
    if not bool(full.any()):
        return 0
    s2 = torch.where(torch.isnan(s[full]), torch.full_like(s[full], float("-inf")), s[full]).clamp(-BIG, BIG)
    d2 = d[full].double().clamp(-BIG, BIG)                  # (float64 distances: check_lists' own .double() is the identity then)
    return R.check_lists(d2, loc[full], s2, k, metric, tag, scale=scale, cap=cap)
