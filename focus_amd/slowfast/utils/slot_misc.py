"""The slot visualisation of the reference's slowfast/utils/slot_misc.py (:16-35): the video that the STEVE loops hand to
the TensorBoard writer's add_video.  The reference module imports cv2, pandas and torchvision at the top; this one needs
torch alone.  On the device the whole video is one launch of csrc/slot_vis.hip (focus_amd.ops.slot_vis_grid); on CPU
tensors it is the reference's loop, with torchvision's make_grid restated below."""
import math

import torch

PAD_VALUE = 0.8                                                      # slot_misc.py:30


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for the case visualize() uses: a 4-D [N,C,H,W] batch with N > 1, no normalisation ->
    [C, ymaps (H + padding) + padding, xmaps (W + padding) + padding] with xmaps = min(nrow, N), ymaps = ceil(N / xmaps);
    image k lies at row k // xmaps, column k % xmaps of the grid, `padding` pixels of pad_value between and around the
    images.  One-channel images are repeated to three, as torchvision does.  Torch expressions: any device."""
    if not torch.is_tensor(tensor) or tensor.dim() != 4:
        raise TypeError("make_grid takes a 4-D tensor [N,C,H,W]; got %s" % (
            tuple(tensor.shape) if torch.is_tensor(tensor) else type(tensor),))
    if tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def visualize_loop(video, recon_dvae, recon_tf, attns, num_slots=4, N=8):
    """slot_misc.py:16-35 as written: per frame one cat and one make_grid.  Any device."""
    B, T, C, H, W = video.size()
    frames = []
    for t in range(T):
        video_t = video[:N, t, None, :, :, :]
        recon_dvae_t = recon_dvae[:N, t, None, :, :, :]
        recon_tf_t = recon_tf[:N, t, None, :, :, :]
        attns_t = attns[:N, t, :, :, :, :]
        tiles = torch.cat((video_t, recon_dvae_t, recon_tf_t, attns_t), dim=1).flatten(end_dim=1)
        frames += [make_grid(tiles, nrow=(num_slots + 3), pad_value=PAD_VALUE)]
    return torch.stack(frames, dim=0).unsqueeze(0)


def visualize(video, recon_dvae, recon_tf, attns, num_slots=4, N=8):
    """The reference's signature: video, recon_dvae [B,T,3,H,W], recon_tf [>= min(N,B),T,3,H,W], attns = the overlays
    [B,T,K,3,H,W] -> frames [1,T,3,Hg,Wg] fp32.  CPU tensors take the loop above.  Device tensors take the kernel, which gives
    the loop's bits for the call the reference makes (num_slots == K, one grid row per clip); what the kernel does not take
    (another num_slots, strided tensors, other dtypes) is a ValueError there, not a slower path."""
    if not video.is_cuda:
        return visualize_loop(video, recon_dvae, recon_tf, attns, num_slots, N)
    from focus_amd import ops
    if attns.dim() == 6 and attns.shape[2] != num_slots:
        raise ValueError("visualize on the device lays out one clip per grid row: num_slots %d is not the K = %d of attns %s" % (
            num_slots, attns.shape[2], tuple(attns.shape)))
    return ops.slot_vis_grid(video, recon_dvae, recon_tf, attns_vis=attns, rows=N)


def visualize_slots(video, recon_dvae, recon_tf, attn, grid, N=8, out_dtype=torch.float32):
    """visualize() from the slot update's own attention: attn [B,T,He*We,K] (fp32 or bf16, what STEVE.forward(..., attns="raw")
    returns) and grid = (He, We) in place of the [B,T,K,3,H,W] overlays, which are never made -- the kernel upsamples and
    blends while it writes the tiles.  out_dtype=torch.uint8 gives the bytes TensorBoard's add_video would make of the fp32
    frames.  Device tensors only: there is no CPU fallback (visualize() on the overlays is the CPU path)."""
    from focus_amd import ops
    return ops.slot_vis_grid(video, recon_dvae, recon_tf, attn=attn, grid=grid, rows=N, out_dtype=out_dtype)
