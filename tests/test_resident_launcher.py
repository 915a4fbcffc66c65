"""`python -m desed_task_amd.launcher ... --resident_data` from a plain shell -- here through tests/launcher_emu.py (the same main() on a
CPU device with the fiber-emulator build of the kernels bound), over the miniature DESED of tests/mini_desed.py: the reference's data
sets are read ONCE into device pools, every training and validation batch is gathered from them.

Not compared against a run without the flag: mini_desed has clips longer than `pad_to`, whose random crop a resident set draws once, at
the read (the documented snapshot deviation)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.test_ddp_gloo import RECIPE, REF, ROOT


def _run(cmd, tmp, env):
    r = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.timeout(1500)
@pytest.mark.skipif(not os.path.isdir(RECIPE), reason="needs the reference's data pipeline (build container only)")
def test_resident_data_cli_trains_validates_checkpoints_and_resumes(tmp_path):
    import yaml
    sys.path[:0] = [p for p in (RECIPE, os.path.join(ROOT, "desed_task_amd", "drop_in"), ROOT, REF) if p not in sys.path]
    from tests import mini_desed
    tmp = str(tmp_path)
    stubs = mini_desed.write_stubs(os.path.join(tmp, "stubs"))
    conf = mini_desed.build(tmp, RECIPE, n_epochs=2)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = os.pathsep.join([RECIPE, os.path.join(ROOT, "desed_task_amd", "drop_in"), ROOT, REF, stubs])
    env["SED_EMU_THREADS"] = "1"            # in-order workgroups: two runs from one seed are arithmetically identical
    base = [sys.executable, "-W", "ignore", "-m", "tests.launcher_emu", "--conf_file", conf, "--gpus", "1", "--resident_data"]
    ckpts = []
    for run in ("a", "b"):
        log_dir = os.path.join(tmp, "exp_" + run)
        out = _run(base + ["--log_dir", log_dir], tmp, env)
        # the first line names pool size and storage: 6 synthetic + 9 of the 10 weak + 8 unlabelled clips, 4 + 1 for validation
        # (weak_split 0.9); mini_desed's stand-in waveforms are no 16-bit PCM, so they stay fp32
        m = re.match(r"resident data: train 23 clips, (\d+) bytes \(audio float32, labels uint8, mask bool\); validation 5 clips, (\d+) bytes "
                     r"\(audio float32, labels uint8, mask bool\)\n", out)
        assert m, out[:400]
        assert int(m.group(1)) == 23 * (16000 * 4 + 160 + 16) and int(m.group(2)) == 5 * (16000 * 4 + 160 + 16)
        assert "epoch 0: 4 steps x 1 ranks" in out and "epoch 1: 4 steps x 1 ranks" in out and out.count("val/obj_metric") >= 2
        assert "best model:" in out
        vdir = os.path.join(log_dir, "version_0")
        files = sorted(os.listdir(vdir))
        assert "last.ckpt" in files and len([f for f in files if f.startswith("epoch=")]) == 1, files
        ckpts.append(torch.load(os.path.join(vdir, "last.ckpt"), map_location="cpu", weights_only=False))
    a, b = ckpts
    assert a["epoch"] == 2 and a["global_step"] == 8 and int(a["optimizer_states"][0]["state"][0]["step"]) == 8
    # two runs with the flag from one seed: bit-identical checkpoints
    assert sorted(a["state_dict"]) == sorted(b["state_dict"])
    for k in a["state_dict"]:
        assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0]["state"], b["optimizer_states"][0]["state"]
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"]), i
    assert a["callbacks"] == b["callbacks"]
    # resume with the flag taken from the YAML this time: one more epoch on top of last.ckpt
    cfg = yaml.safe_load(open(conf))
    cfg["training"]["n_epochs"] = 3
    cfg["training"]["resident_data"] = True
    conf3 = os.path.join(tmp, "conf3.yaml")
    yaml.safe_dump(cfg, open(conf3, "w"))
    out = _run(base[:5] + ["--conf_file", conf3, "--gpus", "1", "--log_dir", os.path.join(tmp, "exp_resumed"), "--resume_from_checkpoint",
                           os.path.join(tmp, "exp_a", "version_0", "last.ckpt")], tmp, env)
    assert out.startswith("resident data: train 23 clips") and "epoch 2: 4 steps x 1 ranks" in out and "epoch 0:" not in out
    c = torch.load(os.path.join(tmp, "exp_resumed", "version_0", "last.ckpt"), map_location="cpu", weights_only=False)
    assert c["epoch"] == 3 and c["global_step"] == 12
    w = "sed_student.cnn.cnn.conv0.weight"
    assert not torch.equal(c["state_dict"][w], a["state_dict"][w])
