#!/usr/bin/env python3
"""test_quant.py with a per-layer weight bit plan on the command line: every flag of test_quant.py plus --bit-plan.

    python -m adalog_amd.utils.bitplan --model deit_small --config ./configs/4bit.py --avg-bits 4 --out plan.json
    python quant_mixed.py --model deit_small --config ./configs/4bit.py --calibrate --bit-plan plan.json

The plan (an adalog-bitplan-v1 file of adalog_amd/utils/bitplan.py, or a bare JSON object of Linear names and widths) is set on
the config as `w_bit_plan` before the model is wrapped; wrap_modules_in_net gives every named layer's weight quantiser its width
and everything after it -- calibration, BRECQ, validation, checkpoints -- reads the width from the quantiser.  A config that sets
`w_bit_plan` itself needs no flag and works through test_quant.py as well; the flag overrides the config.  The flow is
test_quant.main(): its wrap_modules_in_net call is given the plan here.  A mixed checkpoint is reloaded with the same plan
(--bit-plan on the packed, report, gptq and bias_correct tools, or build_wrapped(bit_plan=...)).
"""
import argparse

import test_quant


def with_plan(wrap, plan):
    """wrap_modules_in_net with cfg.w_bit_plan set to ``plan`` first"""
    def wrap_with_plan(model, cfg, reparam=False):
        cfg.w_bit_plan = dict(plan)
        return wrap(model, cfg, reparam=reparam)
    return wrap_with_plan


if __name__ == "__main__":
    parser = argparse.ArgumentParser(parents=[test_quant.get_args_parser()])
    parser.add_argument('--bit-plan', default=None,
                        help="per-layer weight widths: an adalog-bitplan-v1 file of adalog_amd.utils.bitplan "
                             "(default: the config's w_bit_plan, else cfg.w_bit everywhere)")
    args = parser.parse_args()
    if args.bit_plan is not None:
        from adalog_amd.utils.packed import load_bit_plan
        test_quant.wrap_modules_in_net = with_plan(test_quant.wrap_modules_in_net, load_bit_plan(args.bit_plan))
    del args.bit_plan
    test_quant.main(args)
