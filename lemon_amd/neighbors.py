"""The per-sample loop of run_lemon.py:238-307 as one device call per split."""
import ctypes

import torch

from . import _lib
from .index import IndexFlatIP, IndexFlatL2
from .ops import dev_f32, metric_id, paired_distance, ptr, stream_ptr

REC_KEYS = ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m")


def prefix_record(rec, k):
    """The record of a `k` search from the record of a deeper one: an exact best-first list is a prefix of every deeper
    exact list, and dropping the self match (position 0 where the sample is in the DB, else the last position) leaves ranks
    1..K or 0..K-1, whose first k columns are what a k search keeps ("k sweep").  d_1 (and anything else
    that is not a per-neighbour array) passes through as it is; the first k columns of the six neighbour arrays, and of
    I_n / I_m when present, are made contiguous."""
    k = int(k)
    depth = rec["D_n"].shape[1]
    if not 1 <= k <= depth:
        raise ValueError(f"prefix_record: k = {k} is outside 1 .. {depth}, the depth of the record")
    return {key: (v[:, :k].contiguous() if key in REC_KEYS and key != "d_1" else v) for key, v in rec.items()}


class LemonDB:
    """DB side of run_lemon.py:163-176: normalised train embeddings, the two flat indices and
    dists_tr.  Everything stays in HBM."""

    def __init__(self, emb_img_tr, emb_txt_tr, dist_type="cosine", tr_label_id=None, algo=None):
        # dist_type = ("cosine", "euclidean"): the metric sweep -- ONE pair of IP indices serves both metrics
        # (neighbors_metrics); `neighbors` is then the cosine call.  A plain string is one metric, as ever.
        self.metrics = None
        if isinstance(dist_type, (tuple, list)):
            names = tuple("cosine" if metric_id(m) == _lib.METRIC_IP else "euclidean" for m in dist_type)
            if sorted(names) != ["cosine", "euclidean"]:
                raise ValueError(f"a metric sweep takes both of cosine and euclidean, once each; got {dist_type!r}")
            self.metrics, dist_type = names, "cosine"
        self._algo, self._l2 = algo, None
        self.metric = metric_id(dist_type)
        self.img = dev_f32(emb_img_tr, "emb_img_tr")
        self.txt = dev_f32(emb_txt_tr, "emb_txt_tr")
        assert self.img.shape == self.txt.shape and self.img.dim() == 2
        self.device = self.img.device
        cls = IndexFlatIP if self.metric == _lib.METRIC_IP else IndexFlatL2
        d = self.img.shape[1]
        with torch.cuda.device(self.device):
            self.index_img, self.index_txt = cls(d, self.device), cls(d, self.device)   # :167-168 / :171-172
            if algo is not None:
                self.index_img.set_algo(algo)
                self.index_txt.set_algo(algo)
            self.dists_tr = paired_distance(self.metric, self.txt, self.img)            # :169 / :173
            self.index_txt.add(self.txt)                                                # :175
            self.index_img.add(self.img)                                                # :176
            self.dists_tr_l2 = paired_distance(_lib.METRIC_L2, self.txt, self.img) if self.metrics else None   # :173
        self.tr_label_id = None if tr_label_id is None else \
            torch.as_tensor(tr_label_id).to(device=self.device, dtype=torch.int32).contiguous()

    @property
    def ntotal(self):
        return self.img.shape[0]

    def neighbors(self, q_img, q_txt, k, drop_self=False, in_db=None, discrete=False, q_label_id=None,
                  return_indices=True):
        """One split of the scoring loop.  Returns a dict of CUDA tensors keyed like the reference's
        per-sample record (run_lemon.py:291-307) plus I_n / I_m."""
        q_img, q_txt = dev_f32(q_img, "q_img"), dev_f32(q_txt, "q_txt")
        nq, d = q_img.shape
        assert q_txt.shape == (nq, d) and d == self.img.shape[1]
        dev = self.device
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = {"d_1": f(nq)}
        for nm in ("D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
            out[nm] = f(nq, k)
        if return_indices:
            out["I_n"] = torch.empty((nq, k), dtype=torch.int64, device=dev)
            out["I_m"] = torch.empty((nq, k), dtype=torch.int64, device=dev)
        in_db_t = None
        if drop_self and in_db is not None:
            in_db_t = torch.as_tensor(in_db).to(device=dev, dtype=torch.uint8).contiguous()
        q_lab = None
        if discrete:
            if self.tr_label_id is None or q_label_id is None:
                raise ValueError("use_discrete_for_text needs tr_label_id and q_label_id")
            q_lab = torch.as_tensor(q_label_id).to(device=dev, dtype=torch.int32).contiguous()
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.lemon_neighbors(
                self.index_img._h, self.index_txt._h, ptr(self.dists_tr), ptr(q_img), ptr(q_txt), nq, int(k),
                int(bool(drop_self)), ptr(in_db_t), int(bool(discrete)), ptr(self.tr_label_id), ptr(q_lab),
                ptr(out["d_1"]), ptr(out["D_n"]), ptr(out["dists_n"]), ptr(out["dists_tr_n"]), ptr(out.get("I_n")),
                ptr(out["D_m"]), ptr(out["dists_m"]), ptr(out["dists_tr_m"]), ptr(out.get("I_m")),
                stream_ptr(dev)), "lemon_neighbors")
        return out

    def l2_pair(self):
        """The IndexFlatL2 pair over the same tensors that serves the rows a metric sweep cannot certify: built on first
        need and kept."""
        if self._l2 is None:
            self._l2 = LemonDB(self.img, self.txt, "euclidean", tr_label_id=self.tr_label_id, algo=self._algo)
        return self._l2

    def neighbors_metrics(self, q_img, q_txt, k, drop_self=False, in_db=None, discrete=False, q_label_id=None,
                          return_indices=True, margin=4):
        """`neighbors` for both metrics from one search a side ("Metric sweep"): returns
        ({"cosine": rec, "euclidean": rec}, counts).  Each record equals, bit for bit, the one `neighbors` of a LemonDB of
        that dist_type returns.  The euclidean lists are derived from the cosine lists searched `margin` neighbours deeper
        and certified row by row; a row whose image or text side is not certified (ties at the k-th distance: duplicates,
        class prompts, tight clusters) is searched again on `l2_pair()` and scattered back.  counts: rows, certified_n,
        certified_m (rows whose image / text side was certified), fallback (rows searched again) and the per-row flags
        cert_n / cert_m (bool [nq]) those numbers count."""
        if self.metrics is None:
            raise ValueError("neighbors_metrics needs LemonDB(..., dist_type=('cosine', 'euclidean'))")
        margin = int(margin)
        if margin < 0:
            raise ValueError(f"margin must be >= 0, got {margin}")
        q_img, q_txt = dev_f32(q_img, "q_img"), dev_f32(q_txt, "q_txt")
        nq, d = q_img.shape
        assert q_txt.shape == (nq, d) and d == self.img.shape[1]
        dev = self.device
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        recs = {}
        for m in ("cosine", "euclidean"):
            out = {"d_1": f(nq)}
            for nm in ("D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
                out[nm] = f(nq, k)
            if return_indices:
                out["I_n"] = torch.empty((nq, k), dtype=torch.int64, device=dev)
                out["I_m"] = torch.empty((nq, k), dtype=torch.int64, device=dev)
            recs[m] = out
        in_db_t = None
        if drop_self and in_db is not None:
            in_db_t = torch.as_tensor(in_db).to(device=dev, dtype=torch.uint8).contiguous()
        q_lab = None
        if discrete:
            if self.tr_label_id is None or q_label_id is None:
                raise ValueError("use_discrete_for_text needs tr_label_id and q_label_id")
            q_lab = torch.as_tensor(q_label_id).to(device=dev, dtype=torch.int32).contiguous()
        cert_n = torch.zeros((nq,), dtype=torch.uint8, device=dev)
        cert_m = torch.zeros((nq,), dtype=torch.uint8, device=dev)
        outs = []
        for m in ("cosine", "euclidean"):
            o = recs[m]
            outs += [ptr(o["d_1"]), ptr(o["D_n"]), ptr(o["dists_n"]), ptr(o["dists_tr_n"]), ptr(o.get("I_n")),
                     ptr(o["D_m"]), ptr(o["dists_m"]), ptr(o["dists_tr_m"]), ptr(o.get("I_m"))]
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.lemon_neighbors_metrics(
                self.index_img._h, self.index_txt._h, ptr(self.dists_tr), ptr(self.dists_tr_l2), ptr(q_img), ptr(q_txt), nq,
                int(k), int(bool(drop_self)), ptr(in_db_t), int(bool(discrete)), ptr(self.tr_label_id), ptr(q_lab), margin,
                *outs, ptr(cert_n), ptr(cert_m), stream_ptr(dev)), "lemon_neighbors_metrics")
            rows = torch.nonzero((cert_n & cert_m) == 0).flatten()      # (one host synchronisation a call)
            if rows.numel():
                fb = self.l2_pair().neighbors(q_img[rows], q_txt[rows], k, drop_self=drop_self,
                                              in_db=None if in_db_t is None else in_db_t[rows], discrete=discrete,
                                              q_label_id=None if q_lab is None else q_lab[rows], return_indices=return_indices)
                for key, v in fb.items():
                    recs["euclidean"][key][rows] = v
        counts = {"rows": int(nq), "certified_n": int(cert_n.sum()), "certified_m": int(cert_m.sum()),
                  "fallback": int(rows.numel()), "cert_n": cert_n.bool(), "cert_m": cert_m.bool()}
        return recs, counts
