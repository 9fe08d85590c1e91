"""The captured training step's hand-offs (segger_amd.train_step_graph): the loss inputs of a batch are prepared once,
whether the batch is run eagerly, staged, or both; what the forward owes to the end of the step reaches it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(cuda):
    from segger_amd.synthetic import SyntheticSpec
    from tests.test_gpu_train_graph import _model
    return _model(SyntheticSpec(n_tx=5000, n_bd=170, k_tx=7, seed=31), cuda, torch.float32)


@pytest.mark.parametrize("eager_first", [True, False], ids=["eager_then_staged", "staged_then_eager"])
def test_eager_step_and_staging_share_one_preparation_of_the_loss_inputs(cuda, monkeypatch, eager_first):
    """A batch without a persistent store: ``sg_of_tx`` (``ops.anchor_index``) and the boundary loss mask are built by
    whichever of the two comes first, and found by the other."""
    from segger_amd import ops
    from segger_amd.graph import batch_cache
    from segger_amd.train_step_graph import GraphedTrainStep, step_bucket
    m, bg = _setup(cuda)
    assert batch_cache(bg).get("persistent") is None
    built, real = [], ops.anchor_index
    monkeypatch.setattr(ops, "anchor_index", lambda *a, **k: (built.append(1), real(*a, **k))[1])
    step = GraphedTrainStep(m, m.configure_optimizers(capturable=True), step_bucket(bg), bg)

    def eager():
        m.training_step(bg, 0).backward()                 # (the eager loss head asks for sg_of_tx in its backward)

    def masks():
        return [k for k in batch_cache(bg) if isinstance(k, tuple) and k[0] == "bd_loss_mask"]
    first, second = (eager, lambda: step.stage(bg)) if eager_first else (lambda: step.stage(bg), eager)
    first()
    assert len(built) == 1 and len(masks()) == 1
    second()
    assert len(built) == 1, "the second route built sg_of_tx again"
    assert len(masks()) == 1
    step.stage(bg)
    assert len(built) == 1 and len(masks()) == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("merged", [True, False], ids=["merged_draws", "separate_draws"])
def test_every_step_advances_the_dropout_counter_and_adam_once(cuda, monkeypatch, merged, capture):
    """What ``_run_grads`` owes to the end of the step (the dropout counter's advance, whether Adam's counters already
    moved) arrives in ``_opt_step``: after each of three steps, 256 per step and one Adam step per step."""
    from segger_amd import train_step_graph as tsg
    monkeypatch.setattr(tsg, "MERGED_DRAWS", merged)
    m, bg = _setup(cuda)
    opt = m.configure_optimizers(capturable=True)
    step = tsg.GraphedTrainStep(m, opt, tsg.step_bucket(bg, granularity=1.3), bg)
    first = next(iter(m.parameters()))
    for steps in (1, 2, 3):
        out = step.step(bg, capture=capture)
        assert torch.isfinite(out).all()
        assert int(m.model._step_dev) == 256 * steps
        assert float(opt.state[first]["step"]) == steps
    assert (step.graph is not None) == capture
