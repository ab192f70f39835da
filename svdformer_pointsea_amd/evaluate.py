"""The two evaluation protocols of the reference: the per-category CD / DCD / F-Score table.

  evaluate_pcn   core/test_pcn.py:46-105   partial -> model -> [CD-L1 x 1e3, DCD, F1] per sample
  evaluate_55    core/test_55.py:46-101    eight fixed viewpoints x {easy, median, hard} crop of gt,
                                           fps_subsample to 2048 -> model -> [CD-L2 x 1e3, DCD, F1]
  format_table   the text table both scripts print
  AverageMeter   utils/average_meter.py's interface (update / val / count / avg)

The reference runs batch size 1, one forward per view, calc_cd + calc_dcd (the Chamfer search twice,
~50 small launches) and three .item() syncs per forward.  Here
  * any batch size: in eval mode samples are independent, so a batch of B gives B per-sample triples
    (what B forwards at batch 1 give); the eight views of a ShapeNet-55 shape are eight rows of one
    batch (seprate_point_cloud(centers=...));
  * the triple comes from metrics.completion_metrics: one Chamfer search, one launch;
  * bookkeeping stays on the device: triples are added with index_add_ into a float64 tensor of
    per-taxonomy sums and counts (one row [3 sums, count] per taxonomy), the taxonomy index built on
    the host from the ids; no .item(), no sync in the loop, one device-to-host copy at the end;
  * graph=True captures the per-batch step once, for the first batch shape, into static input
    buffers and replays it for every batch of that shape; a last batch of another size runs eagerly.
"""
import torch

from .data import seprate_point_cloud
from .metrics import completion_metrics
from .model_utils import fps_subsample

METRICS = ("CD", "DCD", "F1")
# core/test_55.py:46-53
CROP_RATIO_55 = {"easy": 1 / 4, "median": 1 / 2, "hard": 3 / 4}
VIEWPOINTS_55 = ((1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1))


class AverageMeter:
    """Running value / sum / count of one quantity (items None) or of a named list of them."""

    def __init__(self, items=None):
        self.items = items
        self.n_items = 1 if items is None else len(items)
        self.reset()

    def reset(self):
        self._val = [0] * self.n_items
        self._sum = [0] * self.n_items
        self._count = [0] * self.n_items

    def update(self, values):
        for i, v in enumerate(values if isinstance(values, list) else [values]):
            self._val[i] = v
            self._sum[i] += v
            self._count[i] += 1

    def _get(self, f, idx):
        if idx is not None:
            return f(idx)
        return f(0) if self.items is None else [f(i) for i in range(self.n_items)]

    def val(self, idx=None):
        return self._get(lambda i: self._val[i], idx)

    def count(self, idx=None):
        return self._get(lambda i: self._count[i], idx)

    def avg(self, idx=None):
        return self._get(lambda i: self._sum[i] / self._count[i], idx)


class _Tally:
    """Per-taxonomy sums and counts on the device, one float64 (rows, 4) tensor [3 sums, count] that is
    never reallocated (a captured graph adds into it); rows in order of first appearance."""

    def __init__(self, device, rows=1024):
        self.device = device
        self.rows = {}
        self.acc = torch.zeros(rows, 4, dtype=torch.float64, device=device)

    def index(self, taxonomy_ids, repeat=1):
        """(len(ids) * repeat,) int64 row index on the device, each id `repeat` times in a row."""
        idx = []
        for t in taxonomy_ids:
            t = t if isinstance(t, str) else (t.item() if hasattr(t, "item") else t)
            idx.extend([self.rows.setdefault(t, len(self.rows))] * repeat)
        if len(self.rows) > self.acc.shape[0]:
            raise RuntimeError(f"more than {self.acc.shape[0]} taxonomies")
        return torch.tensor(idx, dtype=torch.int64).to(self.device, non_blocking=True)

    def add(self, index, triples):
        self.acc.index_add_(0, index, torch.cat([triples, torch.ones_like(triples[:, :1])], 1))

    def result(self, protocol):
        acc = self.acc[:len(self.rows)].cpu()   # the one device-to-host copy
        sums, counts = acc[:, :3], acc[:, 3].round().long()
        res = {"protocol": protocol, "metrics": list(METRICS), "taxonomies": {}}
        for t, r in self.rows.items():
            res["taxonomies"][t] = {"count": int(counts[r]), "avg": (sums[r] / counts[r]).tolist()}
        res["overall"] = {"count": int(counts.sum()), "avg": (sums.sum(0) / counts.sum()).tolist()}
        if protocol == "55":
            res["mean_class"] = (sums / counts.unsqueeze(1)).mean(0).tolist()
        return res


def _triples(res, cd):
    """(B, 3) float64 [cd x 1e3, dcd, f1]: the reference scales the Python float (.item() * 1e3)."""
    t = torch.stack((cd, res.dcd, res.f1), 1).double()
    t[:, 0] *= 1e3
    return t


def _loop(step, tally, feed, graph):
    """tally.add(index, step(*inputs)) for every (index, inputs) of `feed`; with `graph`, the first
    batch's shapes are captured (step + add, over static copies of index and inputs) and replayed."""
    static = captured = None
    for index, inputs in feed:
        if not graph or not index.is_cuda:
            tally.add(index, step(*inputs))
            continue
        shapes = [t.shape for t in (index, *inputs)]
        if captured is None:
            static = [t.clone() for t in (index, *inputs)]
            side = torch.cuda.Stream(device=index.device)
            side.wait_stream(torch.cuda.current_stream(index.device))
            with torch.cuda.stream(side):
                for _ in range(2):
                    step(*static[1:])
            torch.cuda.current_stream(index.device).wait_stream(side)
            captured = torch.cuda.CUDAGraph()
            with torch.cuda.graph(captured):
                tally.add(static[0], step(*static[1:]))
            captured.replay()   # capturing ran nothing: this is the first batch
        elif shapes == [t.shape for t in static]:
            for s, t in zip(static, (index, *inputs)):
                s.copy_(t, non_blocking=True)
            captured.replay()
        else:
            tally.add(index, step(*inputs))


def _device_of(model, device):
    if device is not None:
        return torch.device(device)
    p = next(model.parameters(), None)
    return p.device if p is not None else torch.device("cpu")


def _float(t, device):
    return t.to(device, torch.float32, non_blocking=True).contiguous()


def evaluate_pcn(model, batches, images, device=None, graph=False):
    """core/test_pcn.py:46-105.  batches: (taxonomy_ids, model_ids, {'partial_cloud', 'gtcloud'}) as
    datasets.py's collate produces; images(partial) -> the model's image input (PCViews.get_img(...)
    .unsqueeze(1) for SVDFormer, PCViews_Real.get_img for PointSea).  -> the result dict
    {'taxonomies': {id: {'count', 'avg': [CD-L1 x 1e3, DCD, F1]}}, 'overall': {...}}."""
    device = _device_of(model, device)
    model.eval()
    tally = _Tally(device)

    def step(partial, gt):
        pred = model(partial, images(partial))[-1]
        res = completion_metrics(pred.float().contiguous(), gt)
        return _triples(res, res.cd_p)

    def feed():
        for taxonomy_ids, _, data in batches:
            yield tally.index(taxonomy_ids), (_float(data["partial_cloud"], device), _float(data["gtcloud"], device))

    with torch.no_grad():
        _loop(step, tally, feed(), graph)
    return tally.result("pcn")


def evaluate_55(model, batches, images, mode, device=None, graph=False):
    """core/test_55.py:46-101.  batches: (taxonomy_ids, model_ids, {'gtcloud'}); mode: 'easy' / 'median' /
    'hard' (1/4, 1/2, 3/4 of the gt's points cut away around each of the eight fixed viewpoints).  Every
    shape contributes eight triples [CD-L2 x 1e3, DCD, F1]; its eight views are eight rows of one batch.
    -> the result dict of evaluate_pcn plus 'mean_class'."""
    device = _device_of(model, device)
    model.eval()
    tally = _Tally(device)
    views = torch.tensor(VIEWPOINTS_55, dtype=torch.float32, device=device)
    V = len(VIEWPOINTS_55)

    def step(gt):
        B, npoints, _ = gt.shape
        gt8 = gt.repeat_interleave(V, 0)                      # shape 0's eight views, then shape 1's ...
        partial, _ = seprate_point_cloud(gt8, npoints, int(npoints * CROP_RATIO_55[mode]), want_crop=False,
                                         centers=views.repeat(B, 1))
        partial = fps_subsample(partial, 2048).contiguous()
        pred = model(partial, images(partial))[-1]
        res = completion_metrics(pred.float().contiguous(), gt8)
        return _triples(res, res.cd_t)

    def feed():
        for taxonomy_ids, _, data in batches:
            yield tally.index(taxonomy_ids, V), (_float(data["gtcloud"], device),)

    with torch.no_grad():
        _loop(step, tally, feed(), graph)
    return tally.result("55")


def format_table(result):
    """The text both test scripts print (test_pcn.py:82-100, test_55.py:89-101)."""
    head = "============================ TEST RESULTS ============================"
    vals = lambda v: ["%.4f" % x for x in v]   # noqa: E731
    if result["protocol"] == "55":
        lines = [head, "Taxonomy\t#Sample\t" + "\t".join(result["metrics"])]
        for t, r in result["taxonomies"].items():
            lines.append("{:s}\t{:d}\t".format(str(t), r["count"]) + "\t".join(vals(r["avg"])))
        lines.append("Overall\t{:d}\t".format(result["overall"]["count"]) + "\t".join(vals(result["overall"]["avg"])))
        lines.append("MeanClass\t\t" + "\t".join(vals(result["mean_class"])))
        return "\n".join(lines)
    lines = [head, "Taxonomy\t#Sample\t" + "".join(m + "\t" for m in result["metrics"])]
    for t, r in result["taxonomies"].items():
        lines.append("{}\t{}\t".format(t, r["count"]) + "".join(v + "\t" for v in vals(r["avg"])))
    lines.append("Overall\t\t\t" + "".join(v + "\t" for v in vals(result["overall"]["avg"])) + "\n")
    return "\n".join(lines)
