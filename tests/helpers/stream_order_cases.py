"""The table of tests/test_gpu_stream_order.py: every public call of nvimagecodec_amd.lowlevel that takes a `stream`, the checks it gets
(P producer, W no early write, C consumer -- tests/helpers/stalled_stream.py) and the tests that make them.  Needs no device and no
library: tests/test_stream_order_census.py holds it against the classes of lowlevel.py, so a `stream=` parameter added later fails there
until somebody has decided what it promises."""

# "Class.method" -> (checks, tests of tests/test_gpu_stream_order.py)
CASES = {
    "BatchDecoder.decode": ("WC", ("test_decode_writes_behind_the_stream_and_is_seen_by_it", "test_decode_twice_on_one_handle_behind_a_stall")),
    "BatchDecoder.submit": ("WC", ("test_submit_three_batches_behind_one_stall_then_reuse_a_page", "test_submit_on_two_user_streams")),
    "BatchLosslessDecoder.decode": ("WC", ("test_lossless_decode_writes_behind_the_stream_and_is_seen_by_it",
                                           "test_lossless_decode_twice_on_one_handle_behind_a_stall")),
    "BatchEncoder.encode": ("P", ("test_encode_reads_behind_the_stream",)),
    "BatchEncoder.submit": ("P", ("test_encode_submit_three_pages_behind_one_stall_then_reuse_a_page",)),
    "BatchLosslessEncoder.encode": ("P", ("test_lossless_encode_reads_behind_the_stream", "test_lossless_encode_reads_a_padded_input_behind_the_stream")),
    "BatchCoefficients.decode": ("WC", ("test_coefficients_decode_writes_behind_the_stream_and_is_seen_by_it",)),
    "BatchCoefficients.encode": ("P", ("test_coefficients_encode_reads_behind_the_stream",)),
    "BatchCoefficients.to_pixels": ("PWC", ("test_coefficients_to_pixels_in_stream_order",)),
    "BatchCoefficients.from_pixels": ("PWC", ("test_pixels_to_coefficients_in_stream_order",)),
    # a blocking call whose results are host bytes: they are final when it returns, and the stall has ended by then
    "BatchTranscoder.transcode": ("", ("test_transcode_on_a_stalled_stream",)),
}

# "Class.method" -> why it has no test of its own
EXEMPT = {
    "BatchDecoder.transfer": "measurement aid: the copy phase of decode / submit, which are covered",
    "BatchDecoder.device_stage": "measurement aid: the kernel phase of decode / submit, which are covered",
    "BatchEncoder.device_stage": "the device phase of encode, which is covered (encode = device_stage + host_stage)",
    "BatchEncoder.relaunch": "measurement aid: queues the kernels of the last encode again",
    "BatchLosslessDecoder.device_stage": "measurement aid: queues one part of the last decode again",
}

# the plugin's C API takes its streams in nvimgcodecImageInfo_t::cuda_stream, not in a lowlevel method
PLUGIN_CASES = {
    "hipjpeg_decoder (DCT job stream)": ("WC", ("test_plugin_decoder_with_a_user_stream",)),
    "hipjpeg_decoder (lossless stream, gpu_lossless_entropy=1)": ("WC", ("test_plugin_decoder_with_a_user_stream",)),
    "hipjpeg_encoder (baseline and LOSSLESS_HUFFMAN)": ("P", ("test_plugin_encoder_reads_behind_the_user_stream",)),
}
