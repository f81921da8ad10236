#!/usr/bin/env python3
"""Extract the reference's published weak-SINDy (A-WSINDy) runs on the PK/PD EQ_4 family into a JSON fixture.

Source (data, read as text): the ``[Exp evaluation complete] {...}`` log lines the reference's ``run.py:121``
writes in ``/root/reference/results/2_main_table/final_with_insite.txt`` with ``method == 'wsindy'`` and an EQ_4
dataset: one record per dataset and seed (the first such line), its ``global_equation_string``, the RMSE fields
and the line number.  Output: ``tests/golden/reference_log_wsindy.json`` (committed; recorded results only).

    python tests/golden/extract_log_wsindy.py
"""
from __future__ import annotations

import ast
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/results/2_main_table/final_with_insite.txt"
KEYS = ("encoder_test_rmse_all", "encoder_test_rmse_orig", "encoder_test_rmse_last", "decoder_test_rmse_2-step",
        "decoder_test_rmse_3-step", "decoder_test_rmse_4-step", "decoder_test_rmse_5-step",
        "decoder_test_rmse_6-step", "global_equation_string", "method", "seed")


def main():
    marker = "[Exp evaluation complete] "
    out = {}
    with open(SRC) as f:
        for no, line in enumerate(f, 1):
            if marker not in line:
                continue
            rec = ast.literal_eval(line.split(marker, 1)[1].strip())
            ds = rec.get("dataset_name", "")
            if rec.get("method") != "wsindy" or "EQ_4" not in ds:
                continue
            key = f"{ds}/wsindy/{rec.get('seed')}"
            if key not in out:
                out[key] = {"source": f"results/2_main_table/final_with_insite.txt:{no}",
                            **{k: rec[k] for k in KEYS if k in rec}}
    path = os.path.join(HERE, "reference_log_wsindy.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {path}: {sorted(out)}")


if __name__ == "__main__":
    main()
