"""LP_FULL_EVAL / LP_FULL_FILTER through the cfg runner: the Cora
job prints the full evaluation after the last epoch; without the key the
report is today's; outside ALGORITHM:LINKPREDSAMPLE the keys are refused."""
import re

import pytest

from conftest import GOLDEN


def _cora_cfg(tmp_path, extra=""):
    cora = GOLDEN / "cora"
    cfg = tmp_path / "lp_cora.cfg"
    cfg.write_text(
        "ALGORITHM:LINKPREDSAMPLE\nVERTICES:2708\nLAYERS:1433-64-32\nFANOUT:10-5\nBATCH_SIZE:512\n"
        "EPOCHS:2\nLEARN_RATE:0.01\nWEIGHT_DECAY:0.0001\nDROP_RATE:0.1\nNEG_PER_POS:4\n"
        "VAL_EDGE_RATE:0.1\nSEED:2000\n" + extra +
        f"EDGE_FILE:{cora / 'cora.2708.edge.self'}\nFEATURE_FILE:{cora / 'cora.featuretable'}\n"
        f"LABEL_FILE:{cora / 'cora.labeltable'}\nMASK_FILE:{cora / 'cora.mask'}\n")
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [0, 1])
def test_cora_job_prints_the_full_evaluation(tmp_path, filt):
    from nts import run
    lines = []
    res = run.run(_cora_cfg(tmp_path, f"LP_FULL_EVAL:1\nLP_FULL_FILTER:{filt}\n"), out=lines.append)
    print("\n".join(lines))
    full = [l for l in lines if l.startswith("Full Val MRR:")]
    assert len(full) == 1 and lines[-1] == full[0]  # after the last epoch
    m = re.fullmatch(r"Full Val MRR: (\d\.\d{6}) Hits@10: (\d\.\d{6}) \((\d+) edges against 2708 "
                     r"candidates(, filtered)?\)", full[0])
    assert m and bool(m.group(4)) == bool(filt)
    mrr, hits, n = float(m.group(1)), float(m.group(2)), int(m.group(3))
    assert 0.0 < mrr <= 1.0 and 0.0 <= hits <= 1.0 and n == res["n_val_edges"] == 1356
    assert res["full_val"]["mrr"] == pytest.approx(mrr, abs=1e-6)
    # a trained model on Cora ranks far above chance (1 / V)
    assert mrr > 10.0 / 2708


def test_the_keys_default_to_0_and_are_refused_outside_link_prediction(tmp_path):
    from nts import dataloader, run
    info = dataloader.InputInfo.from_cfg(_cora_cfg(tmp_path))
    assert info.lp_full_eval == 0 and info.lp_full_filter == 0
    run.refuse_link_pred_cfg(info)  # today's cfg passes
    info.algorithm = "GCNSAMPLEALLGPU"
    run.refuse_cfg(info)
    info.lp_full_eval = 1
    with pytest.raises(SystemExit, match="LP_FULL_EVAL is not supported outside ALGORITHM:LINKPREDSAMPLE"):
        run.refuse_cfg(info)
