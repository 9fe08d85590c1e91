"""What the captured training step and the graphed predictor share (segger_amd.capture): the ladder of bucket sizes,
the test of a batch against a bucket, the pool policy and the gradient exchange.  No GPU."""
import types

import pytest
import torch

from segger_amd import capture
from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX

# (granularity, floor) -> [(n, size, size with one granule of headroom)], computed once from the ladder code as it stood
# before the two ladders became one: step_bucket's ``up(n)`` / ``up(n, 1)``, bucket_sizes' ``up(n)`` and the predictor
# pool's ``int(size * g) + 1`` loop.  Per row: 0, floor - 1, floor, floor + 1, the fifth rung -1 / exactly / +1, 1e6.
LADDER = {
    (1.06, 256): [(0, 256, 272), (255, 256, 272), (256, 272, 289), (257, 272, 289),
                  (345, 346, 367), (346, 367, 390), (347, 367, 390), (1000000, 1036624, 1098822)],
    (1.06, 1024): [(0, 1024, 1086), (1023, 1024, 1086), (1024, 1086, 1152), (1025, 1086, 1152),
                   (1373, 1374, 1457), (1374, 1457, 1545), (1375, 1457, 1545), (1000000, 1001198, 1061270)],
    (1.08, 256): [(0, 256, 277), (255, 256, 277), (256, 277, 300), (257, 277, 300),
                  (380, 381, 412), (381, 412, 445), (382, 412, 445), (1000000, 1071086, 1156773)],
    (1.08, 1024): [(0, 1024, 1106), (1023, 1024, 1106), (1024, 1106, 1195), (1025, 1106, 1195),
                   (1506, 1507, 1628), (1507, 1628, 1759), (1508, 1628, 1759), (1000000, 1049664, 1133638)],
    (1.25, 256): [(0, 256, 321), (255, 256, 321), (256, 321, 402), (257, 321, 402),
                  (786, 787, 984), (787, 984, 1231), (788, 984, 1231), (1000000, 1245191, 1556489)],
    (1.25, 1024): [(0, 1024, 1281), (1023, 1024, 1281), (1024, 1281, 1602), (1025, 1281, 1602),
                   (3130, 3131, 3914), (3131, 3914, 4893), (3132, 3914, 4893), (1000000, 1036667, 1295834)],
    (1.5, 256): [(0, 256, 385), (255, 256, 385), (256, 385, 578), (257, 385, 578),
                 (1954, 1955, 2933), (1955, 2933, 4400), (1956, 2933, 4400), (1000000, 1284995, 1927493)],
    (1.5, 1024): [(0, 1024, 1537), (1023, 1024, 1537), (1024, 1537, 2306), (1025, 1537, 2306),
                  (7786, 7787, 11681), (7787, 11681, 17522), (7788, 11681, 17522), (1000000, 1010501, 1515752)],
}
TRAIN_EDGES = {"e_tt": TX_TX, "e_tb": TX_BD}
PREDICT_EDGES = {"__".join(et): et for et in (TX_TX, TX_BD, TX_NB_BD)}


class _Batch(dict):
    """Counts only: what the ladder, ``fits`` and ``waste`` read of a batch."""
    def __init__(self, tx, bd, edges, num_graphs=1):
        node = lambda n: types.SimpleNamespace(num_nodes=n)
        super().__init__({"tx": node(tx), "bd": node(bd)})
        for et, n in edges.items():
            self[et] = types.SimpleNamespace(edge_index=types.SimpleNamespace(shape=(2, n)))
        self.num_graphs = num_graphs


def _uniform(n):
    return _Batch(n, n, {TX_TX: n, TX_BD: n, TX_NB_BD: n}, num_graphs=n)


@pytest.mark.parametrize("key", list(LADDER), ids=lambda k: f"g{k[0]}-floor{k[1]}")
def test_one_ladder_gives_the_sizes_of_both_steps(key):
    from segger_amd.inference import bucket_sizes
    from segger_amd.train_step_graph import step_bucket
    g, floor = key
    tt = "__".join(TX_TX)
    for n, size, roomy in LADDER[key]:
        assert n < size < roomy
        assert capture.ladder(n, g, floor) == size and capture.ladder(n, g, floor, 1) == roomy
        b = _uniform(n)
        assert step_bucket(b, g, floor) == {"tx": size, "bd": roomy, "e_tt": size, "e_tb": roomy, "graphs": roomy}
        plain, head = bucket_sizes(b, g, floor), bucket_sizes(b, g, floor, headroom=1)
        assert list(plain) == ["tx", "bd", *PREDICT_EDGES] and list(head) == list(plain)
        assert all(v == size for v in plain.values())
        assert all(v == (size if k in ("tx", tt) else roomy) for k, v in head.items())


def test_ladder_defaults_are_the_two_steps_own():
    from segger_amd.inference import bucket_sizes
    from segger_amd.train_step_graph import step_bucket
    b = _uniform(1025)
    assert step_bucket(b) == step_bucket(b, 1.06, 256) and bucket_sizes(b) == bucket_sizes(b, 1.25, 1024, 0)


@pytest.mark.parametrize("edges,e_tt", [(TRAIN_EDGES, "e_tt"), (PREDICT_EDGES, "__".join(TX_TX))], ids=["train", "predict"])
def test_a_batch_fits_below_node_sizes_and_up_to_edge_and_graph_sizes(edges, e_tt):
    sizes = {"tx": 100, "bd": 20, "graphs": 4, **{k: 300 + i for i, k in enumerate(edges)}}
    def batch(**over):
        c = {"tx": 99, "bd": 19, "graphs": 4, **{k: sizes[k] for k in edges}, **over}
        return _Batch(c["tx"], c["bd"], {et: c[k] for k, et in edges.items()}, c["graphs"])
    assert capture.fits(sizes, batch(), edges)                      # node size - 1, edge size, graph size: all fit
    assert capture.counts(batch(), edges) == {"tx": 99, "bd": 19, "graphs": 4, **{k: sizes[k] for k in edges}}
    for nt in ("tx", "bd"):
        assert not capture.fits(sizes, batch(**{nt: sizes[nt]}), edges)     # no room for the dummy
    for k in edges:
        assert not capture.fits(sizes, batch(**{k: sizes[k] + 1}), edges)
    assert not capture.fits(sizes, batch(graphs=5), edges)
    b = _Batch(1, 1, {et: 1 for et in edges.values()})
    delattr(b, "num_graphs")
    assert capture.fits(sizes, b, edges)                            # a batch without num_graphs is one graph
    # waste: the larger of the tx ratio and the tx-neighbors-tx edge ratio; nothing else counts, empty counts as 1
    assert capture.waste(sizes, batch(tx=50, **{e_tt: 100}), edges, e_tt) == sizes[e_tt] / 100
    assert capture.waste(sizes, batch(tx=10, **{e_tt: 100}), edges, e_tt) == 100 / 10
    assert capture.waste(sizes, batch(tx=50, bd=1, **{e_tt: 300, [k for k in edges if k != e_tt][0]: 1}), edges, e_tt) == 2.0
    assert capture.waste(sizes, batch(tx=0, **{e_tt: 0}), edges, e_tt) == float(sizes[e_tt])


def test_both_classes_answer_with_the_shared_shape_test():
    from segger_amd.inference import GraphedPredictor
    from segger_amd.train_step_graph import GraphedTrainStep
    step, pred = object.__new__(GraphedTrainStep), object.__new__(GraphedPredictor)
    step.sizes = {"tx": 100, "bd": 20, "e_tt": 300, "e_tb": 40, "graphs": 4}
    pred.sizes = {"tx": 100, "bd": 20, **{k: 300 for k in PREDICT_EDGES}}
    pred._limits = {**pred.sizes, "graphs": 4}
    for bucket in (step, pred):
        e = lambda tt, tb=40: {TX_TX: tt, TX_BD: tb, TX_NB_BD: 300}
        assert bucket.fits(_Batch(99, 19, e(300), 4)) and bucket.waste(_Batch(50, 19, e(100), 4)) == 3.0
        assert not bucket.fits(_Batch(100, 19, e(300), 4)) and not bucket.fits(_Batch(99, 20, e(300), 4))
        assert not bucket.fits(_Batch(99, 19, e(301), 4)) and not bucket.fits(_Batch(99, 19, e(300), 5))
    assert not step.fits(_Batch(99, 19, {TX_TX: 300, TX_BD: 41}, 4))
    assert not pred.fits(_Batch(99, 19, {TX_TX: 300, TX_BD: 300, TX_NB_BD: 301}, 4))


class _Bucket:
    def __init__(self, holds, waste):
        self._holds, self._waste = holds, waste

    def fits(self, batch):
        return self._holds

    def waste(self, batch):
        return self._waste


def test_pool_policy():
    g = 1.5
    made = []
    def make():
        made.append(_Bucket(True, 1.0))
        return made[-1]
    pick = lambda pool, max_buckets=8: capture.pick(pool, "batch", make, g, max_buckets, "pool is full")
    tight = _Bucket(True, 1.2)
    pool = [_Bucket(True, 2.0), _Bucket(False, 1.0), tight, _Bucket(True, 1.3)]
    assert capture.tightest(pool, "batch") is tight and pick(pool) is tight and not made and len(pool) == 4
    assert capture.tightest([_Bucket(False, 1.0)], "batch") is None
    # a fit that wastes more than two granules: a new bucket below max_buckets, used as it is at max_buckets
    loose = _Bucket(True, g ** 2 + 0.01)
    pool = [loose]
    assert pick(pool, max_buckets=1) is loose and not made
    assert pick(pool, max_buckets=2) is made[0] and pool == [loose, made[0]] and len(made) == 1
    pool = [_Bucket(True, g ** 2)]                        # exactly two granules is still tight enough
    assert pick(pool) is pool[0] and len(made) == 1
    # nothing fits: a new bucket, or an error with the caller's text once the pool is full
    pool = [_Bucket(False, 1.0)]
    assert pick(pool, max_buckets=2) is made[1] and len(pool) == 2 and len(made) == 2
    pool = [_Bucket(False, 1.0)]
    with pytest.raises(RuntimeError, match="pool is full"):
        pick(pool, max_buckets=1)
    assert len(made) == 2 and len(pool) == 1
    assert pick([]) is made[2] and len(made) == 3        # the first batch of an empty pool


def test_the_two_pools_keep_their_own_error_text():
    from segger_amd.inference import GraphedPredictorPool
    from segger_amd.train_step_graph import GraphedTrainer
    tr, pool = GraphedTrainer(None, None, max_buckets=1), GraphedPredictorPool(None, 4, max_buckets=1)
    tr.buckets.append(_Bucket(False, 1.0))
    pool.buckets.append(_Bucket(False, 1.0))
    with pytest.raises(RuntimeError, match="no captured bucket holds this batch and 1 buckets exist: raise `granularity`"):
        tr.step(_uniform(10))
    with pytest.raises(RuntimeError, match="no captured bucket holds this batch and 1 buckets exist$"):
        pool.predict(_uniform(10))
    assert tr.n_captures == 0 and len(tr.buckets) == 1 and len(pool.buckets) == 1


# ------------------------------------------------------------------------------------------------ the gradient exchange
class _Graph:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def replay(self):
        self.log.append(self.name)


class _FlatBucket:
    """The part of dp.FlatGradBucket the exchange uses, counting."""
    def __init__(self, params, log):
        self.params, self.views, self.log = params, [torch.ones_like(p) for p in params], log

    def pack(self):
        self.log.append("pack")

    def zero(self):
        self.log.append("zero")
        for p, v in zip(self.params, self.views):
            v.zero_()
            p.grad = v

    def all_reduce_mean(self, packed=False):
        assert packed
        self.log.append("reduce")


def _split_step(exchange, params, grads, log):
    from segger_amd.train_step_graph import GraphedTrainStep
    step = object.__new__(GraphedTrainStep)
    step.exchange, step.split = exchange, exchange.split
    step.graph, step.graph_opt = _Graph(log, "backward"), _Graph(log, "adam")
    step._params, step._grads = params, grads
    return step


@pytest.mark.parametrize("mode", ["none", "callable", "bucket", "bucket_method"])
def test_every_exchange_mode_reduces_once_per_step_and_per_empty_step(mode):
    from segger_amd.train_step_graph import GraphedTrainer
    params = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    grads = [torch.full_like(p, 7.0) for p in params]
    log, seen = [], []
    def sync():
        log.append("reduce")
        seen.append([p.grad for p in params])
    bucket = _FlatBucket(params, log)
    ex = capture.exchange_of(*{"none": (None, None), "callable": (sync, None), "bucket": (None, bucket),
                               "bucket_method": (bucket.all_reduce_mean, None)}[mode])
    assert ex.split == (mode != "none") and (ex.bucket is bucket) == mode.startswith("bucket")
    assert (ex.sync is sync) == (mode == "callable")
    step = _split_step(ex, params, grads, log)
    step._replay()
    assert log == (["backward"] if mode == "none" else ["backward", "reduce", "adam"])
    given = bucket.views if mode.startswith("bucket") else grads
    if mode != "none":
        assert all(p.grad is g for p, g in zip(params, given))         # Adam reads what the backward graph wrote
    if mode == "callable":
        assert all(a is b for a, b in zip(seen[-1], grads))            # ... and the callable reduced exactly those
    del log[:]
    if mode != "none":
        step._replay(empty=True)
        assert log == (["reduce", "adam"] if mode == "callable" else ["zero", "reduce", "adam"])
        assert all(p.grad is g and not g.any() for p, g in zip(params, given))     # zeros went into the exchange
        if mode == "callable":
            assert all(a is b for a, b in zip(seen[-1], grads))
    # the trainer's empty step before anything was captured on this rank: eager, still one reduce, then the optimizer
    del log[:]
    for p in params:
        p.grad = None
    frozen = torch.nn.Parameter(torch.ones(1), requires_grad=False)
    opt = types.SimpleNamespace(param_groups=[{"params": params + [frozen]}], step=lambda: log.append("opt.step"))
    tr = GraphedTrainer(None, opt, grad_sync=ex.sync, grad_bucket=ex.bucket)
    assert tr.step(None) is None
    if mode == "none":
        assert log == [] and all(p.grad is None for p in params)
    else:
        assert log == (["reduce", "opt.step"] if mode == "callable" else ["zero", "reduce", "opt.step"])
        assert all(p.grad is not None and not p.grad.any() for p in params) and frozen.grad is None
        if mode == "callable":
            assert all(a is p.grad for a, p in zip(seen[-1], params))
    # ... and through the last captured step once there is one
    del log[:]
    tr._last, step.opt = step, opt
    tr.step(None)
    if mode != "none":
        assert log.count("reduce") == 1 and log[-1] == "adam" and "backward" not in log
