"""The host logic of ``fit_loop.run`` on CPU tensors, with a toy fit and ``ops.clip_adam`` replaced
by a recorder (as tests/test_octree_dist_cpu.py replaces ``ops``): the steps, the epochs, the report
steps, the printed line and the log; ``report_line`` and ``check_schedule`` on their own."""

import math
import re
import types

import pytest
import torch

from fourier_feature_nets_amd import fit_loop


class _Toy:
    """A fit of three batches an epoch that writes down, in order, everything the loop calls."""

    def __init__(self, monkeypatch, batches=(10, 11, 12)):
        self.events, self.batches, self.epochs = [], list(batches), 0
        self.data = torch.zeros((5, 3))
        monkeypatch.setattr(fit_loop, "ops", types.SimpleNamespace(clip_adam=self.clip_adam))

    def epoch(self):
        self.epochs += 1
        return [(self.epochs, batch) for batch in self.batches]

    def step(self, batch, grads):
        assert grads.shape == self.data.shape and grads.dtype == self.data.dtype
        self.events.append(("step", batch))
        grads.fill_(float(batch[1]))
        return torch.tensor(0.5 * len([e for e in self.events if e[0] == "step"]))

    def clip_adam(self, flat, grads, exp_avg, exp_avg_sq, number, learning_rate, clip_value,
                  max_norm, scratch):
        assert flat.data_ptr() == self.data.data_ptr() and flat.shape == (15,)
        assert grads.shape == exp_avg.shape == exp_avg_sq.shape == (15,)
        assert scratch.numel() == 1 and scratch.dtype == torch.float32
        self.events.append(("adam", number, learning_rate, clip_value, max_norm,
                            float(grads[0]), float(exp_avg.abs().sum())))
        exp_avg += 1                      # the moments are the loop's own, kept from step to step
        flat -= 1.0

    def project(self, data):
        assert data is self.data
        self.events.append(("project",))

    def validate(self):
        self.events.append(("validate",))
        return 20.0 + len(self.events)

    def run(self, num_steps, validate=True, report_interval=4, verbose=False, fields=None):
        return fit_loop.run(self.data, self.epoch, self.step, self.project,
                            self.validate if validate else None, num_steps, 2.5e-3,
                            report_interval, 0.3, 0.7, verbose, fields)

    def of(self, kind):
        return [event for event in self.events if event[0] == kind]


def test_no_steps_call_nothing(monkeypatch, capsys):
    toy = _Toy(monkeypatch)
    assert toy.run(0, verbose=True) == []
    assert toy.events == [] and toy.epochs == 0 and capsys.readouterr().out == ""


def test_steps_epochs_and_the_order_within_a_step(monkeypatch):
    toy = _Toy(monkeypatch)
    log = toy.run(7, validate=False)
    assert [entry.step for entry in log] == list(range(7))
    assert all(isinstance(entry, fit_loop.FitLogEntry) for entry in log)
    assert [entry.loss for entry in log] == [0.5 * (k + 1) for k in range(7)]
    # three batches an epoch: a fresh epoch() after each one runs out, and the run stops at the
    # first batch of the third
    assert toy.epochs == 3
    assert [event[1] for event in toy.of("step")] == [(1, 10), (1, 11), (1, 12), (2, 10), (2, 11),
                                                      (2, 12), (3, 10)]
    # every step: the caller's step, K7 with the step number k + 1 on its gradient, the projection
    assert [event[0] for event in toy.events] == ["step", "adam", "project"] * 7
    for k, event in enumerate(toy.of("adam")):
        assert event[1:5] == (k + 1, 2.5e-3, 0.3, 0.7)
        assert event[5] == float(toy.of("step")[k][1][1]) and event[6] == 15.0 * k
    assert toy.data.eq(-7.0).all()


def test_a_run_that_ends_with_its_epoch_asks_for_no_further_one(monkeypatch):
    toy = _Toy(monkeypatch)
    assert len(toy.run(6, validate=False)) == 6
    assert toy.epochs == 2 and len(toy.of("step")) == 6


def test_report_steps(monkeypatch, capsys):
    toy = _Toy(monkeypatch)
    log = toy.run(26, report_interval=12)
    reported = [entry.step for entry in log if math.isfinite(entry.val_psnr)]
    assert reported == list(range(10)) + [12, 24]
    assert all(math.isnan(entry.val_psnr) for entry in log if entry.step not in reported)
    assert len(toy.of("validate")) == 12
    # validation sees the projected data of its own step
    at = toy.events.index(("validate",))
    assert [event[0] for event in toy.events[:at + 1]] == ["step", "adam", "project", "validate"]
    assert log[0].val_psnr == 24.0
    assert capsys.readouterr().out == ""                       # verbose is off

    silent = _Toy(monkeypatch)
    log = silent.run(13, validate=False, report_interval=12, verbose=True,
                     fields=lambda: [("never", 0.0)])
    assert len(log) == 13 and all(math.isnan(entry.val_psnr) for entry in log)
    assert silent.of("validate") == [] and capsys.readouterr().out == ""


LINE = re.compile(r"^(\d{7}) (\d+\.\d{6}) s/step loss: (\d+\.\d{6}) val_psnr: (\d+\.\d{6}) "
                  r"first: 1\.500000 second: -2\.000000 lr: 2\.50e-03 eta: (.+)$")


def test_the_printed_lines(monkeypatch, capsys):
    toy = _Toy(monkeypatch)
    log = toy.run(9, report_interval=4, verbose=True,
                  fields=lambda: [("first", 1.5), ("second", -2.0)])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 9
    for k, line in enumerate(lines):
        found = LINE.match(line)
        assert found, line
        assert int(found.group(1)) == k
        assert float(found.group(3)) == log[k].loss
        assert float(found.group(4)) == pytest.approx(log[k].val_psnr, abs=1e-6)
        if k < 4:
            assert found.group(2) == "0.000000" and found.group(5) == "N/A"
        else:
            assert re.fullmatch(r"[A-Z][a-z]{2}, \d{2} [A-Z][a-z]{2} \d{4} \d{2}:\d{2}:\d{2} \+0000",
                                found.group(5)), line

    plain = _Toy(monkeypatch)
    plain.run(1, verbose=True)
    assert re.fullmatch(r"0000000 0\.000000 s/step loss: 0\.500000 val_psnr: \d+\.\d{6} "
                        r"lr: 2\.50e-03 eta: N/A\n", capsys.readouterr().out)


def test_report_line_on_its_own():
    line = fit_loop.report_line(500, 2000, 500, 100.0, 150.0,
                                [("psnr_train", 21.25), ("val_psnr", 20.5)], 5e-4)
    # 0.1 s/step, 1500 steps to go: 150 s after ``now``
    assert line == ("0000500 0.100000 s/step psnr_train: 21.250000 val_psnr: 20.500000 "
                    "lr: 5.00e-04 eta: Thu, 01 Jan 1970 00:05:00 +0000")
    early = fit_loop.report_line(499, 2000, 500, 100.0, 150.0, [("loss", 0.125)], 1e-2)
    assert early == "0000499 0.000000 s/step loss: 0.125000 lr: 1.00e-02 eta: N/A"


def test_refusals_carry_the_callers_name():
    rule = "batch_size >= 1, num_steps >= 0, report_interval >= 1"
    fit_loop.check_schedule("fit_toy", rule, 1, 0, 1, 1e-2)
    for batch, num_steps, report_interval in ((0, 5, 1), (1, -1, 1), (1, 5, 0)):
        with pytest.raises(ValueError) as caught:
            fit_loop.check_schedule("fit_toy", rule, batch, num_steps, report_interval, 1e-2)
        assert str(caught.value) == "fit_toy: " + rule
    for rate in (0.0, -1e-2, float("nan")):
        with pytest.raises(ValueError, match=r"^fit_toy: learning_rate must be positive, got "):
            fit_loop.check_schedule("fit_toy", rule, 1, 5, 1, rate)


def test_the_log_entry_is_one_type_under_every_name():
    import fourier_feature_nets
    import fourier_feature_nets_amd
    from fourier_feature_nets_amd import mesh, octree_fit
    assert octree_fit.FitLogEntry is fit_loop.FitLogEntry
    assert fourier_feature_nets_amd.FitLogEntry is fit_loop.FitLogEntry
    assert fourier_feature_nets.FitLogEntry is fit_loop.FitLogEntry
    assert mesh.fit_loop is fit_loop and octree_fit.fit_loop is fit_loop
