"""Data-side contract of the hot path: what a clip and its boxes go through between
decoding and `model(inputs, meta)` -- spatial sampling WITH boxes, pathway packing and the `orvit_bboxes` wire format.
RandAugment, spatial sampling and random erasing also run on the device (device_sampling.make_batch).  Decoding, samplers and
the dataset classes themselves stay the reference's."""
