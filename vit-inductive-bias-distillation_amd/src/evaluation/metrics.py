"""Drop-in for ``evaluate_model`` of the reference's ``src/evaluation/metrics.py`` (same module path and name):
``from src.evaluation.metrics import evaluate_model`` as in reference ``src/training/trainer.py``.  The dataset and
efficiency helpers of that module (``measure_efficiency``, ``run_eval_suite``) have no counterpart here."""
from basd_amd.evaluation import EvalAccumulator, evaluate_model  # noqa: F401
