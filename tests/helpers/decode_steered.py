"""Test helper (run as a child process, so that the library's switches apply -- they are read once per process): the steered files of
helpers/steered_streams.py with placed stuffed bytes and restart markers (seams, chunk seams, last chunks, restart markers), each family
as one batch through the GPU entropy stage, compared with the oracle's pixels."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

FAMILIES = ("seams", "chunks", "last_chunk", "restart_placed")


def main():
    from helpers import steered_streams as S
    from nvimagecodec_amd.lowlevel import BatchDecoder
    dec = BatchDecoder(device=0, num_threads=4)
    files = 0
    for name in FAMILIES:
        S.decode_on_device(dec, S.family(name))
        files += len(S.family(name))
    dec.close()
    print("steered ok", files)


if __name__ == "__main__":
    main()
