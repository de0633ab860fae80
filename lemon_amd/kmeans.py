"""k-means on caption embeddings, on the device (lemon_amd/csrc/kmeans.hip).

  FaissKMeans(n_clusters, n_init, max_iter, seed).fit / predict      lib/datasets/clustering.py:13-41
  cluster_caption_text(clip_model, text_list, n_clusters)            lib/datasets/clustering.py:69-75

The host does only what faiss does on the host: the sub-sample when n > max_points_per_centroid * C, the seeded choice of
the initial centroids of every redo and the choice of the best redo.  Everything per iteration -- assignment, float64
centroid means, the empty-cluster split -- is enqueued by ONE lemon_kmeans_train call per redo and the host synchronises
once per redo to read its objective.

NOT faiss's random streams: the sub-sample is the first max_points_per_centroid * C entries of
np.random.RandomState(seed).permutation(n), redo r starts from the first C rows of
np.random.RandomState(seed + r).permutation(n_train), and an empty cluster takes half of the LARGEST cluster (faiss draws the
donor at random).  Centroids are not re-normalised (faiss spherical=False).
"""
import numpy as np
import torch

from . import _lib
from .ops import dev_f32, normalize_vectors, ptr, stream_ptr

MAX_CLUSTERS = 16384
MAX_DIM = 1024


def _check(x, c):
    assert x.dim() == 2 and c.dim() == 2 and x.shape[1] == c.shape[1], (tuple(x.shape), tuple(c.shape))
    assert x.device == c.device


def assign(x, centroids, return_dist=True, out=None):
    """Nearest centroid of every row: (assign int32 [n], dist float32 [n]) == IndexFlatL2(d).add(centroids).search(x, 1).
    `out`: caller-provided (assign, dist) buffers to write into."""
    x, c = dev_f32(x, "x"), dev_f32(centroids, "centroids")
    _check(x, c)
    if out is not None:
        a, dist = out
        assert a.dtype == torch.int32 and a.is_contiguous() and a.shape[0] == x.shape[0] and a.device == x.device
        assert dist is None or (dist.dtype == torch.float32 and dist.is_contiguous() and dist.shape[0] == x.shape[0])
        return_dist = dist is not None
    else:
        a = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        dist = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if return_dist else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().lemon_kmeans_assign(ptr(x), x.shape[0], x.shape[1], ptr(c), c.shape[0], ptr(a), ptr(dist),
                                                   stream_ptr(x.device)), "lemon_kmeans_assign")
    return (a, dist) if return_dist else a


def _workspace(n, d, C, device):
    nbytes = int(_lib.load().lemon_kmeans_workspace_bytes(n, d, C))
    if nbytes < 0:
        _lib.check(nbytes, "lemon_kmeans_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def update(x, assignment, dist, centroids):
    """One centroid step IN PLACE on `centroids` (float32 CUDA, contiguous): returns (count int64 [C], obj float64 [1])."""
    x = dev_f32(x, "x")
    _check(x, centroids)
    assert centroids.dtype == torch.float32 and centroids.is_contiguous()
    C = centroids.shape[0]
    a = assignment.to(device=x.device, dtype=torch.int32).contiguous()
    dist = dev_f32(dist, "dist")
    assert a.shape[0] == x.shape[0] == dist.shape[0]
    count = torch.empty(C, dtype=torch.int64, device=x.device)
    obj = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = _workspace(x.shape[0], x.shape[1], C, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().lemon_kmeans_update(ptr(x), x.shape[0], x.shape[1], ptr(a), ptr(dist), C, ptr(centroids), ptr(count),
                                                   ptr(obj), ptr(ws), ws.numel(), stream_ptr(x.device)), "lemon_kmeans_update")
    return count, obj


def split_empty(centroids, count):
    """The empty-cluster rule IN PLACE on `centroids` (float32) and `count` (int64), both CUDA and contiguous."""
    assert centroids.dtype == torch.float32 and centroids.is_contiguous() and count.dtype == torch.int64 and count.is_contiguous()
    with torch.cuda.device(centroids.device):
        _lib.check(_lib.load().lemon_kmeans_split(ptr(centroids), centroids.shape[1], centroids.shape[0], ptr(count),
                                                  stream_ptr(centroids.device)), "lemon_kmeans_split")


def train(x, init_centroids, niter):
    """One redo of Lloyd's iteration from `init_centroids`, enqueued without a host synchronisation: returns
    (centroids float32 [C, d], obj_hist float64 [niter], count int64 [C], assign int32 [n]), all on the device."""
    x = dev_f32(x, "x")
    c = dev_f32(init_centroids, "init_centroids").clone()
    _check(x, c)
    n, d, C = x.shape[0], x.shape[1], c.shape[0]
    obj = torch.empty(max(int(niter), 1), dtype=torch.float64, device=x.device)
    count = torch.zeros(C, dtype=torch.int64, device=x.device)
    a = torch.empty(n, dtype=torch.int32, device=x.device)
    ws = _workspace(n, d, C, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().lemon_kmeans_train(ptr(x), n, d, C, int(niter), ptr(c), ptr(obj), ptr(count), ptr(a), ptr(ws),
                                                  ws.numel(), stream_ptr(x.device)), "lemon_kmeans_train")
    return c, obj[:int(niter)], count, a


def subsample_rows(n, n_clusters, max_points_per_centroid, seed):
    """Row numbers the fit trains on: all of them, or -- when n > max_points_per_centroid * C, as faiss does -- that many
    drawn without replacement (the head of a seeded permutation, in permutation order)."""
    cap = int(max_points_per_centroid) * int(n_clusters)
    if n <= cap:
        return None
    return np.random.RandomState(seed).permutation(n)[:cap]


def initial_rows(n_train, n_clusters, seed, redo):
    """Rows of the training matrix that seed redo `redo`: the first C entries of a permutation seeded with seed + redo."""
    return np.random.RandomState(seed + redo).permutation(n_train)[:n_clusters]


class KMeans:
    """The FaissKMeans surface (clustering.py:13-41) on the device.  `fit(X)` takes a numpy array or a torch tensor [n, d];
    `predict(X)` returns int64 [n, 1] like index.search(X, 1)[1] (numpy in -> numpy out, CUDA tensor in -> CUDA tensor out) and
    embeds a list of strings first when an `embed_func` was given."""

    def __init__(self, n_clusters=8, n_init=5, max_iter=300, seed=42, max_points_per_centroid=1024, device=None,
                 embed_func=None):
        if not 1 <= int(n_clusters) <= MAX_CLUSTERS:
            raise ValueError(f"n_clusters must lie in [1, {MAX_CLUSTERS}], got {n_clusters}")
        if int(n_init) < 1 or int(max_iter) < 1:
            raise ValueError("n_init and max_iter must be at least 1")
        self.n_clusters, self.n_init, self.max_iter, self.seed = int(n_clusters), int(n_init), int(max_iter), int(seed)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.device, self.embed_func = device, embed_func
        self.cluster_centers_ = self.inertia_ = self.obj_ = None
        self.best_redo_ = self.n_train_ = None
        self._centers_dev = None

    def _to_dev(self, X):
        device = self.device
        if device is None:
            device = X.device if torch.is_tensor(X) and X.is_cuda else torch.device("cuda", torch.cuda.current_device())
        t = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)) if isinstance(X, np.ndarray) else X
        return t.to(device=device, dtype=torch.float32).contiguous()

    def fit(self, X):
        x = self._to_dev(X)
        n, d = x.shape
        if n < self.n_clusters:
            raise ValueError(f"{n} points cannot seed {self.n_clusters} clusters")
        if d % 4 or not 4 <= d <= MAX_DIM:
            raise ValueError(f"the embedding width must be a multiple of 4 in [4, {MAX_DIM}], got {d}")
        # a NaN row is at "distance 0" from every centroid (the key clamps with dd > 0 ? dd : 0), joins cluster 0 and turns
        # its mean into NaN, which then attracts every point: refuse here, as raise_if_nonfinite does on the dataset path
        if not bool(torch.isfinite(x).all()):
            raise ValueError("KMeans.fit: the input holds non-finite values (NaN or Inf)")
        rows = subsample_rows(n, self.n_clusters, self.max_points_per_centroid, self.seed)
        if rows is not None:
            x = x[torch.from_numpy(rows).to(x.device)].contiguous()
        self.n_train_ = int(x.shape[0])
        best = None
        for redo in range(self.n_init):
            init = x[torch.from_numpy(initial_rows(self.n_train_, self.n_clusters, self.seed, redo)).to(x.device)]
            c, obj, _, _ = train(x, init, self.max_iter)
            obj = obj.cpu().numpy()                       # the one synchronisation of this redo
            if best is None or obj[-1] < best[1][-1]:     # ties: the earlier redo
                best = (c, obj, redo)
        self._centers_dev, self.obj_, self.best_redo_ = best
        self.cluster_centers_ = self._centers_dev.cpu().numpy()
        self.inertia_ = float(self.obj_[-1])
        return self

    def predict(self, X):
        if isinstance(X, (list, tuple)):
            if self.embed_func is None:
                raise TypeError("predict() on strings needs the embed_func the model was built with")
            X = self.embed_func(list(X))
        if self._centers_dev is None:
            raise RuntimeError("predict() before fit()")
        was_numpy = isinstance(X, np.ndarray)
        a = assign(self._to_dev(X).to(self._centers_dev.device), self._centers_dev, return_dist=False)
        out = a.to(torch.int64).unsqueeze(1)
        return out.cpu().numpy() if was_numpy else out


def embed_caption_text(embedder, tokenize, text_list, batch_size=4096):
    """Normalised text embeddings [n, d] (CUDA) of a list of captions: clustering.py:44-66 on the project's text tower
    (`tokenize`: list of strings -> LongTensor [n, context], cli_common.prepare's)."""
    out = []
    for s in range(0, len(text_list), batch_size):
        out.append(embedder.embed_texts(tokenize(list(text_list[s:s + batch_size]))))
    embedder.raise_if_nonfinite()
    d = embedder.model.cfg.embed_dim
    return normalize_vectors(torch.cat(out)) if out else torch.empty((0, d), device=embedder.device)


def make_tokenize(tokenizer, device=None):
    """The two tokenizer conventions of lib/models/utils.py:64-105 as one list-of-strings -> LongTensor [n, context]
    function: the HF tokenizer is called with padding="max_length", truncation=True and returns a dict of lists
    (clustering.py:58-60), the in-tree ones return the id tensor themselves (:54).  With `device` and LEMON_TOKENIZE=device
    the tokenizer's device form is returned where it has one (tokenizer.device_form: the same ids, on the GPU)."""
    from .tokenizer import device_form, tokenize_mode
    on_device = device_form(tokenizer, device) if device is not None and tokenize_mode() == "device" else None
    if on_device is not None:
        return on_device

    def tokenize(prompts):
        try:
            enc = tokenizer(prompts, padding="max_length", truncation=True)
        except TypeError:
            enc = tokenizer(prompts)
        return torch.tensor(enc["input_ids"]) if hasattr(enc, "keys") else enc
    return tokenize


def cluster_caption_text(embedder, tokenizer, text_list, n_clusters=100, random_state=42, **kmeans_kwargs):
    """clustering.py:69-75: embed the captions, normalise, fit, predict -> (km, labels int64 [n] on the host).
    `tokenizer`: the tokenizer algorithm_class_from_scratch returns, or any list-of-strings -> LongTensor callable."""
    tokenizer = make_tokenize(tokenizer, embedder.device)
    emb = embed_caption_text(embedder, tokenizer, text_list)
    km = KMeans(n_clusters=n_clusters, seed=random_state, device=emb.device,
                embed_func=lambda texts: embed_caption_text(embedder, tokenizer, texts), **kmeans_kwargs)
    km.fit(emb)
    return km, km.predict(emb).squeeze(1).cpu().numpy()
