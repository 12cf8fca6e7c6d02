"""Pixels of one image as a 2-D regression dataset (reference: pixel_dataset.py:14-198).

Names, signatures, the uv convention (0..2 from ``meshgrid``, training pixels ``[::2, ::2]``) and
the outputs of ``to_image`` / ``to_act_image`` / ``generate_uvs`` / ``psnr`` follow the reference.
Differences: targets are float32 (the reference keeps float64 on the host), a pre-lifted (N,3)
copy of the uvs feeds ``RegressionEngine`` (``train_uv3`` / ``val_uv3``), and ``from_array``
builds a dataset from pixels in memory.

cv2 is not available here.  ``create`` decodes with PIL, centre-crops, resizes by area averaging
(the block mean with round-half-up, as cv2.INTER_AREA computes it for integer ratios; other
ratios use PIL's box filter: parity unpinned, like the Dilate ellipse) and converts to YCrCb with
``utils.rgb_to_ycrcb_u8``.  The decode itself is PIL's, also unpinned.  YCrCb -> RGB of u8
frames runs on the GPU (kernel K8b).
"""

import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .utils import check_color_space, rgb_to_ycrcb_u8


class PixelData(NamedTuple("PixelData", [("uv", torch.FloatTensor),
                                         ("color", torch.FloatTensor)])):
    """(uv, color): uv values in 0..2 (..., 2) and colours in 0..1 (..., 3)."""


def _ycrcb_to_rgb(pixels: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(pixels, cv2.COLOR_YCrCb2RGB) on a u8 frame: kernel K8b on a GPU."""
    if not torch.cuda.is_available():
        raise RuntimeError("YCrCb -> RGB runs on the GPU (kernel K8b); there is no CPU fallback")
    frame = torch.from_numpy(np.ascontiguousarray(pixels)).to("cuda")
    ops.ycrcb_to_rgb_u8(frame)
    return frame.cpu().numpy()


def _centre_crop(pixels: np.ndarray) -> np.ndarray:
    rows, cols = pixels.shape[:2]
    if rows > cols:
        start = (rows - cols) // 2
        return pixels[start:start + cols, :]
    if cols > rows:
        start = (cols - rows) // 2
        return pixels[:, start:start + rows]
    return pixels


def _area_resize(pixels: np.ndarray, size: int) -> np.ndarray:
    """Square u8 image -> (size, size): block means for an integer ratio, PIL's box filter
    otherwise (unpinned against cv2.INTER_AREA)."""
    side = pixels.shape[0]
    if side == size:
        return pixels
    if side % size == 0:
        k = side // size
        blocks = pixels.reshape(size, k, size, k, -1).astype(np.int64).sum(axis=(1, 3))
        return ((blocks + (k * k) // 2) // (k * k)).astype(np.uint8)
    from PIL import Image
    return np.asarray(Image.fromarray(pixels).resize((size, size), Image.BOX))


class PixelDataset:
    """Dataset consisting of image pixels."""

    def __init__(self, size: int, color_space: str,
                 train_data: PixelData, val_data: PixelData):
        check_color_space(color_space)
        self.size = size
        self.color_space = color_space
        self.image = self.to_image(val_data.color)
        self.train_uv, self.train_color = train_data
        self.val_uv, self.val_color = val_data
        self._lifted = {}

    @staticmethod
    def from_array(pixels: np.ndarray, color_space: str, size=512) -> "PixelDataset":
        """A dataset from (H,W,3) u8 RGB pixels (not in the reference: no image file needed).
        Crop, resize and colour conversion as ``create``."""
        check_color_space(color_space)
        pixels = np.asarray(pixels)
        if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3:
            raise ValueError("pixels must be (H,W,3) uint8 RGB")
        pixels = _area_resize(_centre_crop(pixels), size)
        if color_space == "YCrCb":
            pixels = rgb_to_ycrcb_u8(pixels)
        colors = pixels.astype(np.float32) / np.float32(255)
        # NB the uv range of 0 to 2, as in the reference (pixel_dataset.py:91-93)
        vals = np.linspace(0, 2, size // 2, endpoint=False, dtype=np.float32)
        train_uv = np.stack(np.meshgrid(vals, vals), axis=-1)
        train_color = np.ascontiguousarray(colors[::2, ::2, :])
        vals = np.linspace(0, 2, size, endpoint=False, dtype=np.float32)
        val_uv = np.stack(np.meshgrid(vals, vals), axis=-1)
        dataset = PixelDataset.__new__(PixelDataset)
        dataset.size = size
        dataset.color_space = color_space
        # the ground-truth frame as the reference derives it: float64 colours -> (x 255) -> u8
        image = (pixels / 255 * 255).astype(np.uint8)
        dataset.image = _ycrcb_to_rgb(image) if color_space == "YCrCb" else image
        dataset.train_uv, dataset.train_color = torch.from_numpy(train_uv), torch.from_numpy(train_color)
        dataset.val_uv, dataset.val_color = torch.from_numpy(val_uv), torch.from_numpy(colors)
        dataset._lifted = {}
        return dataset

    @staticmethod
    def create(path: str, color_space: str, size=512) -> "PixelDataset":
        """Creates a dataset from an image file (decoded with PIL), or returns None (with a
        message) when it cannot be read."""
        check_color_space(color_space)
        if not os.path.exists(path):
            alt = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "data", path))
            if os.path.exists(alt):
                path = alt
        try:
            from PIL import Image
            with Image.open(path) as img:
                pixels = np.asarray(img.convert("RGB"))
        except (OSError, ValueError):
            print("Unable to load image at", path)
            return None
        return PixelDataset.from_array(pixels, color_space, size)

    def to(self, *args) -> "PixelDataset":
        """Equivalent of torch.Tensor.to for all tensors in the dataset."""
        out = PixelDataset.__new__(PixelDataset)
        out.size, out.color_space, out.image = self.size, self.color_space, self.image
        out.train_uv, out.train_color = self.train_uv.to(*args), self.train_color.to(*args)
        out.val_uv, out.val_color = self.val_uv.to(*args), self.val_color.to(*args)
        out._lifted = {}
        return out

    def _lift(self, name: str) -> torch.Tensor:
        uv = getattr(self, name)
        cached = self._lifted.get(name)
        if cached is None or cached[0] is not uv:
            flat = uv.reshape(-1, 2).to(torch.float32)
            cached = (uv, torch.nn.functional.pad(flat, (0, 1)).contiguous())
            self._lifted[name] = cached
        return cached[1]

    @property
    def train_uv3(self) -> torch.Tensor:
        """Training uvs as (N,3) positions with a zero third column (RegressionEngine's input)."""
        return self._lift("train_uv")

    @property
    def val_uv3(self) -> torch.Tensor:
        return self._lift("val_uv")

    @property
    def train_color_flat(self) -> torch.Tensor:
        """(N,3) float32 training colours, rows in ``train_uv3`` order."""
        return self.train_color.reshape(-1, 3)

    @property
    def val_color_flat(self) -> torch.Tensor:
        return self.val_color.reshape(-1, 3)

    def to_act_image(self, model, size: int) -> np.ndarray:
        """Grid of 8 x 8 images: the contribution of each of the first 64 channels of the last
        hidden layer through the output layer (pixel_dataset.py:128-166)."""
        num_grid = 8
        grid_size = size // num_grid
        uvs = self.generate_uvs(grid_size, next(model.parameters()).device)
        uvs = uvs.reshape(-1, 2)
        model.keep_activations = True
        with torch.no_grad():
            model(uvs)
        model.keep_activations = False
        palette = model.layers[-1].weight.data.detach().cpu().numpy()
        bias = model.layers[-1].bias.data.detach().cpu().numpy()
        activation = model.activations[-1].T[..., np.newaxis]
        palette = palette.T[:, np.newaxis, :]
        values = torch.sigmoid(torch.from_numpy(activation * palette + bias)).numpy()
        act_pixels = np.zeros((size, size, 3), np.float32)
        for i in range(num_grid):
            for j in range(num_grid):
                tile = values[i * num_grid + j].reshape(grid_size, grid_size, 3)
                act_pixels[i * grid_size:(i + 1) * grid_size, j * grid_size:(j + 1) * grid_size] = tile
        act_pixels = (act_pixels * 255).astype(np.uint8)
        if self.color_space == "YCrCb":
            act_pixels = _ycrcb_to_rgb(act_pixels)
        return act_pixels

    def to_image(self, colors: torch.Tensor, size=0) -> np.ndarray:
        """Predicted colours (size*size, 3) or (size, size, 3) -> (size, size, 3) u8 RGB image:
        (colors * 255) truncated (pixel_dataset.py:168-192)."""
        if size == 0:
            size = self.size
        pixels = (colors * 255).reshape(size, size, 3).cpu().numpy().astype(np.uint8)
        if self.color_space == "YCrCb":
            pixels = _ycrcb_to_rgb(pixels)
        return pixels

    @staticmethod
    def generate_uvs(size: int, device) -> torch.Tensor:
        """(size, size, 2) uv grid in 0..2 (pixel_dataset.py:194-207)."""
        vals = np.linspace(0, 2, size, endpoint=False, dtype=np.float32)
        uvs = np.stack(np.meshgrid(vals, vals), axis=-1)
        return torch.from_numpy(uvs).to(device=device)

    def psnr(self, colors: torch.Tensor) -> float:
        """Peak signal-to-noise ratio of ``colors`` against the validation colours
        (pixel_dataset.py:209-220)."""
        mse = torch.square(colors.reshape(self.val_color.shape) - self.val_color).mean().item()
        return -10 * math.log10(mse)

    @staticmethod
    def psnr_from_sse(sse: float, count: int) -> float:
        """The same PSNR from a sum of squared errors over ``count`` values (RegressionEngine)."""
        return -10 * math.log10(sse / count)
