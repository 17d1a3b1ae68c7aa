"""Host side of the frame renderer (include/cagpu.h CaRender, csrc/cagpu_render.inc; drawing rules: DESIGN.md section 13).

What is here is everything of a render call that is not a kernel: the palette, the window of a frame, and the FRAME
DESCRIPTORS -- which slots of the trajectory tape a frame shows.  The descriptor functions are torch code without a
device assumption (they run on the tape's device in the product path, on CPU tensors in tests/test_render_host.py) and
never bring a tape row to the host.  Encoding frames as PNG / GIF files (save_frames) goes through PIL.
"""
import os

# envs/visualize.py:18-25: orange, blue, green, purple, yellow, cyan, chocolate -- and as bytes, round(255 c), the table the
# kernel holds
PALETTE = ((0.8500, 0.3250, 0.0980), (0.0, 0.4470, 0.7410), (0.4660, 0.6740, 0.1880), (0.4940, 0.1840, 0.5560),
           (0.9290, 0.6940, 0.1250), (0.3010, 0.7450, 0.9330), (0.6350, 0.0780, 0.1840))
PALETTE8 = tuple(tuple(int(c * 255 + 0.5) for c in rgb) for rgb in PALETTE)
DEFAULT_LIMITS = ((-8.0, 8.0), (-8.0, 8.0))   # the 16 m x 16 m map extent centred on the origin


def window(size, limits=None):
    """(H, W), ((xmin, xmax), (ymin, ymax)) -> xmin, ymax, s16 of CaRender: equal scale on both axes, the largest at which
    the limits fit the frame, the limits' centre in the middle of the frame; s16 = 16 x pixels per metre"""
    H, W = int(size[0]), int(size[1])
    (x0, x1), (y0, y1) = DEFAULT_LIMITS if limits is None else limits
    x0, x1, y0, y1 = float(x0), float(x1), float(y0), float(y1)
    if not (x1 > x0 and y1 > y0):
        raise ValueError("limits %r: need xmin < xmax and ymin < ymax" % (limits,))
    ppm = min(W / (x1 - x0), H / (y1 - y0))
    return (x0 + x1) / 2 - W / (2 * ppm), (y0 + y1) / 2 + H / (2 * ppm), 16 * ppm


def episode_ranges(episode, epoch, cur_episode, cur_epoch, which="current", upto=None):
    """The tape slots of ONE episode per env -> (first, last), int32 [S] each; last < first: none (a snapshot frame).

    episode, epoch: int [T, S], the tape's counters of the selected envs (BatchedSim.trajectories: the auto-reset count as
    a step started, the host-side resets); cur_episode, cur_epoch: int [S], the counters NOW.  An episode is a run of slots
    with one (epoch, episode) pair; the pairs never decrease along the tape, so the running episode's slots are the tape's
    tail and every episode is contiguous.
      which="current": the slots whose pair is the current one (none right after a reset);
      which="last":    the most recent episode before the current one that the tape holds;
      upto=k:          only the episode's slots up to its k-th (0-based)."""
    import torch
    if which not in ("current", "last"):
        raise ValueError("episode must be 'current' or 'last', got %r" % (which,))
    T, S = int(episode.shape[0]), int(episode.shape[1])
    dev = episode.device
    if T == 0:
        return (torch.zeros((S,), dtype=torch.int32, device=dev), torch.full((S,), -1, dtype=torch.int32, device=dev))
    cur = (episode == cur_episode.unsqueeze(0)) & (epoch == cur_epoch.unsqueeze(0))
    ncur = cur.sum(dim=0)
    if which == "current":
        first, last = T - ncur, torch.full_like(ncur, T - 1)
    else:
        tl = T - ncur - 1                       # the last slot of another episode
        has = tl >= 0
        idx = tl.clamp(min=0).unsqueeze(0)
        same = (episode == episode.gather(0, idx)) & (epoch == epoch.gather(0, idx))
        first, last = tl - same.sum(dim=0) + 1, tl
        first, last = torch.where(has, first, torch.zeros_like(first)), torch.where(has, last, torch.full_like(last, -1))
    if upto is not None:
        last = torch.minimum(last, first + max(0, int(upto)))
    return first.to(torch.int32), last.to(torch.int32)


def prefix_lasts(length, every=1):
    """the last row (0-based) of every animation frame of an episode of `length` rows: prefixes of every, 2 every, ... rows
    and the whole episode"""
    every = max(1, int(every))
    lasts = list(range(every - 1, int(length) - 1, every))
    return lasts + [int(length) - 1] if length > 0 else []


def save_frames(path, frames, duration_ms=100, hold_last=10):
    """one frame [H, W, 3] -> a PNG, several [F, H, W, 3] -> an animated GIF whose last frame stays 1 + hold_last times as
    long (the reference appends the final plot ten times, visualize.py:66-67); uint8 numpy arrays, encoded by PIL"""
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("saving frames needs Pillow (PIL) to encode PNG / GIF files; render() / render_episode() return "
                           "the raw uint8 frames without it") from exc
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if frames.ndim == 3:
        Image.fromarray(frames, "RGB").save(path)
        return path
    imgs = [Image.fromarray(f, "RGB") for f in frames]
    durations = [int(duration_ms)] * (len(imgs) - 1) + [int(duration_ms) * (1 + int(hold_last))]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=durations, loop=0)
    return path
