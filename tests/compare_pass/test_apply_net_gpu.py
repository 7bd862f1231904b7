"""apply_net with several --inference-config paths as a command: three configs over four synthetic frames write three result files (and
sidecars) that are, byte for byte, those of three single-config runs on the same topology -- one rank, and two gloo ranks sharing the GPU.
Random-init weights: the plumbing and the identity contract are what is checked.

The module shares its name with tests/test_apply_net_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INFERENCE = os.path.join(ROOT, "pod_compare_amd", "configs", "Inference")
# BayesOD over two MC-dropout runs: a second family beside the single-run configs, at a fifth of the YAML's ten runs
MC2 = ('PROBABILISTIC_INFERENCE:\n  INFERENCE_MODE: "bayes_od"\n  AFFINITY_THRESHOLD: 0.9\n  MC_DROPOUT: {ENABLE: true, NUM_RUNS: 2}\n'
       '  BAYES_OD: {CLS_MERGE_MODE: "max_score", BOX_MERGE_MODE: "bayesian_inference"}\n')
NAMES = ("standard_nms", "bayes_od", "bayes_od_mc2")


def apply_net(cwd, ranks, args):
    cmd = [sys.executable]
    if ranks > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                "--master-port", str(37500 + os.getpid() % 2000)]
    cmd += ["-m", "pod_compare_amd.apply_net", "--num-images", "4", "--random-init", "--random-seed", "7", "--flush-every", "2"] + list(args)
    if ranks > 1:
        cmd += ["--backend", "gloo", "--share-gpu"]
    subprocess.check_call(cmd, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0"), timeout=900)


def read(path):
    with open(str(path), "rb") as f:
        return f.read()


@pytest.mark.parametrize("ranks", [1, 2])
def test_three_configs_write_the_files_of_three_runs(tmp_path, ranks):
    (tmp_path / "bayes_od_mc2.yaml").write_text(MC2)
    paths = [os.path.join(INFERENCE, "standard_nms.yaml"), os.path.join(INFERENCE, "bayes_od.yaml"), str(tmp_path / "bayes_od_mc2.yaml")]
    apply_net(tmp_path, ranks, ["--inference-config"] + paths + ["--binary-output", "results.podr"])
    for name, path in zip(NAMES, paths):
        apply_net(tmp_path, ranks, ["--inference-config", path, "--output", str(tmp_path / (name + ".json")),
                                    "--binary-output", str(tmp_path / (name + ".podr"))])
        shared = tmp_path / "output" / "inference" / "bdd_val" / name
        assert len(read(tmp_path / (name + ".json"))) > 100
        assert read(shared / "coco_instances_results.json") == read(tmp_path / (name + ".json")), name
        assert read(shared / "results.podr") == read(tmp_path / (name + ".podr")), name
    assert read(tmp_path / "standard_nms.json") != read(tmp_path / "bayes_od.json") != read(tmp_path / "bayes_od_mc2.json")


def test_a_single_config_run_writes_the_same_bytes_twice(tmp_path):
    """One path: the command of before (two sessions, the same file)."""
    for name in ("a", "b"):
        apply_net(tmp_path, 1, ["--inference-config", os.path.join(INFERENCE, "bayes_od.yaml"), "--output", str(tmp_path / (name + ".json"))])
    assert len(read(tmp_path / "a.json")) > 100 and read(tmp_path / "a.json") == read(tmp_path / "b.json")
