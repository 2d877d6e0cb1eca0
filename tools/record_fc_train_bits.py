"""Records the bits of the FC-head training kernels (csrc/fc_train.hip): a CRC32 of the raw bytes
of every output (Y, A, stats, the running statistics after the call, dY, dW, dbias, dgamma,
dbeta) of the 64-row and of the any-B entry pair, for the cases of
tests/test_gpu_fc_rows.py::golden_bits (the shapes of SHAPES, BELOW and RULE_CASES plus four
more, each with every BN mode and with and without ReLU, inputs from make_inputs with fixed
seeds).  tests/test_gpu_fc_rows.py::test_bits_are_the_recorded_ones recomputes and compares them.

tests/golden/fc_train_bits.json was produced with the kernels of commit 0abf69a ("Losses,
log_softmax and loop metrics as fixed-order HIP kernels"), the last one with separate one-slab and
slab kernels.  Record again only when an order rule changes on purpose.
Needs a ROCm device.  Writes one JSON document (default tests/golden/fc_train_bits.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_fc_rows as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("record_fc_train_bits: needs a ROCm device")
    crc = T.golden_bits()
    head = {"what": "CRC32 of the raw float32 bytes of each output; key = B,N,K,bn,relu,entry "
                    "(64: pn2_fc_bn_*_f32, rows: pn2_fc_bn_*_rows_f32)",
            "kernels_of_commit": "0abf69a", "device": torch.cuda.get_device_name(0), "cases": len(crc)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:  # a case per line
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
        f.write(' "crc32": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in crc.items()))
        f.write("\n }\n}\n")
    print("record_fc_train_bits: %d cases -> %s" % (len(crc), a.out))


if __name__ == "__main__":
    main()
