#!/usr/bin/env python3
"""test_quant.py with QDrop's switch on the command line: every flag of test_quant.py plus --drop-prob.

    python quant_qdrop.py --model deit_small --config ./configs/4bit.py --calibrate --optimize --drop-prob 0.5

In every BRECQ iteration each activation element keeps its fake-quantised value with probability P and passes through
unquantised otherwise (adalog_amd/quantizers/_drop.py); evaluation always quantises.  A config that sets `drop_prob` needs no
flag and works through test_quant.py as well (wrap_modules_in_net reads it); the flag, 1.0 = off included, overrides the
config.  The flow is test_quant.main(): its reconstruct_model() call gives no probability and takes
BlockReconstructor.drop_prob, which is set here.
"""
import argparse

import test_quant

if __name__ == "__main__":
    parser = argparse.ArgumentParser(parents=[test_quant.get_args_parser()])
    parser.add_argument('--drop-prob', type=float, default=None,
                        help="QDrop: probability that an activation element keeps its quantised value in a BRECQ iteration "
                             "(default: the config's drop_prob, else 1.0 = off; needs train_act)")
    args = parser.parse_args()
    if args.drop_prob is not None:
        if not 0.0 <= args.drop_prob <= 1.0:
            parser.error("--drop-prob must lie in [0, 1]")
        from adalog_amd.utils.block_recon import BlockReconstructor
        BlockReconstructor.drop_prob = float(args.drop_prob)
    del args.drop_prob
    test_quant.main(args)
