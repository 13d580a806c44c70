"""python -m espnet_amd.bin.lm_train — espnet2/bin/lm_train.py (LMTask.main)."""
from __future__ import annotations

from ..tasks.lm import LMTask


def get_parser():
    return LMTask.get_parser()


def main(cmd=None):
    LMTask.main(cmd=cmd)


if __name__ == "__main__":
    main()
