"""detection/model_utils.py:55-116 — the patch classifier's training loop: Adam, StepLR(n_epochs // 2), cross-entropy, and per
epoch the validation accuracy, precision and recall.  The reference reads its loaders, datasets and device from notebook globals
and plots after every epoch; here they are arguments and the histories are returned."""
import numpy as np
import torch
import torch.nn as tnn

from .model import PatchModel


def precision_recall(y_true, y_pred):
    """(precision, recall) of the positive class of two boolean arrays; 0.0 where the denominator is 0 (sklearn's
    precision_score / recall_score with their default zero_division, without the warning)."""
    y_true, y_pred = np.asarray(y_true, dtype=bool), np.asarray(y_pred, dtype=bool)
    tp = int((y_true & y_pred).sum())
    predicted, actual = int(y_pred.sum()), int(y_true.sum())
    return (tp / predicted if predicted else 0.0), (tp / actual if actual else 0.0)


def train(train_dataloader, val_dataloader, n_epochs=20, lr=3e-4, schedule_factor=.1, saving=True, model=None, device="cuda",
          save_path="best_model.pth"):
    """Returns (model, history) with history = dict(train_loss, val_accuracy, precision, recall).  The loaders yield
    (patches (N, 2, 16, 32), labels (N,)) batches.  saving: keep the state_dict of the best validation accuracy in `save_path`
    (the reference compares with a `best_val_accuracy` that it never updates, so it saves every epoch; here the best one is kept)."""
    model = (PatchModel() if model is None else model).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, max(n_epochs // 2, 1), schedule_factor)
    criterion = tnn.CrossEntropyLoss()
    history = dict(train_loss=[], val_accuracy=[], precision=[], recall=[])
    best_val_accuracy = 0
    for epoch in range(n_epochs):
        model.train()
        for batch in train_dataloader:
            X_batch, y_batch = batch[0].to(device, dtype=torch.float32), batch[1].to(device).long()
            loss = criterion(model(X_batch), y_batch)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            history["train_loss"].append(loss.item())
        scheduler.step()

        model.eval()
        correct, seen, y_pred, y_val = 0, 0, [], []
        with torch.no_grad():
            for batch in val_dataloader:
                X_batch, y_batch = batch[0].to(device, dtype=torch.float32), batch[1].to(device).long()
                predicted_labels = torch.argmax(model(X_batch), dim=1)
                correct += (predicted_labels == y_batch).sum().item()
                seen += y_batch.numel()
                y_pred += list(predicted_labels.cpu().numpy())
                y_val += list(y_batch.cpu().numpy())
        history["val_accuracy"].append(correct / max(seen, 1))
        if saving and history["val_accuracy"][-1] > best_val_accuracy:
            best_val_accuracy = history["val_accuracy"][-1]
            torch.save(model.state_dict(), save_path)
        precision, recall = precision_recall(y_val, y_pred)
        history["precision"].append(precision)
        history["recall"].append(recall)
    return model, history
