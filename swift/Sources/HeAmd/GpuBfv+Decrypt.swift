// Decryption of ciphertexts that are resident on the device: Bfv.decryptCoeff / decryptEval (Bfv+Decrypt.swift:21-39),
// Bfv.noiseBudgetCoeff / noiseBudgetEval (:116-185) and Bfv.isTransparent (Bfv+Encrypt.swift:48-62) over a batch
// [batch][polyCount][L][N] -- a server's replies where they were computed.  What comes back is N words mod t per ciphertext,
// or one Double, instead of 2 L N words.
//
// The single-ciphertext HeScheme members of GpuBfv keep forwarding to CpuBfv (GpuBfv.swift): one polynomial across PCIe and
// back costs more than the host's own dot product.
import CHeAmd
import HomomorphicEncryption

extension GpuBfv {
    /// The secret key as the decryption entries read it: [L_all][N] Eval over the secret-key context.  Only the first
    /// rows, those of the ciphertexts' level, are read (PolyRq.swift:184-194).
    public static func residentSecretKey(_ secretKey: SecretKey<GpuBfv>, on stream: HeAmdStream) throws -> DeviceBuffer {
        let buffer = try DeviceBuffer(count: secretKey._poly.data.count)
        try buffer.upload(secretKey._poly, at: 0, on: stream)
        return buffer
    }

    /// `decryptCoeff` / `decryptEval` of `batch` resident ciphertexts over `polyContext`: `plaintexts` receives
    /// [batch][N] values below t.  Enqueue-only; scratch is stream-ordered.
    public static func gpuDecrypt(resident ciphertexts: DeviceBuffer, batch: Int, polyCount: Int,
                                  polyContext: PolyContext<UInt64>, evalFormat: Bool, correctionFactor: UInt64,
                                  secretKey: DeviceBuffer, into plaintexts: DeviceBuffer, context: Context,
                                  on stream: HeAmdStream) throws
    {
        try heAmdCheck(he_bfv_decrypt_device(context.gpu, 64, UInt32(polyContext.moduli.count), UInt32(polyCount),
                                             evalFormat ? 1 : 0, ciphertexts.pointer, secretKey.pointer, correctionFactor,
                                             plaintexts.pointer, batch, nil, 0, stream.raw))
    }

    /// `noiseBudgetCoeff` / `noiseBudgetEval` of `batch` resident ciphertexts: the exact norms are taken on the device, the
    /// stream is waited for, and each norm becomes the reference's Double on the host.
    /// - Warning: The noise budget value **must not** be forwarded to any other party.  Sharing it acts as an oracle that can
    ///   be used to recover the secret key.
    public static func gpuNoiseBudget(resident ciphertexts: DeviceBuffer, batch: Int, polyCount: Int,
                                      polyContext: PolyContext<UInt64>, evalFormat: Bool, secretKey: DeviceBuffer,
                                      variableTime: Bool, context: Context, on stream: HeAmdStream) throws -> [Double]
    {
        let level = UInt32(polyContext.moduli.count)
        let limbs = Int(he_bfv_noise_norm_limbs(context.gpu, level))
        let norms = try DeviceBuffer(count: max(batch * limbs, 1))
        try heAmdCheck(he_bfv_noise_norm_device(context.gpu, 64, level, UInt32(polyCount), evalFormat ? 1 : 0,
                                                ciphertexts.pointer, secretKey.pointer, norms.pointer, batch, nil, 0,
                                                stream.raw))
        var words = [UInt64](repeating: 0, count: batch * limbs)
        try words.withUnsafeMutableBufferPointer { destination in
            try heAmdCheck(he_memcpy_d2h(destination.baseAddress, norms.pointer,
                                         batch * limbs * MemoryLayout<UInt64>.stride, stream.raw))
            try heAmdCheck(he_stream_synchronize(stream.raw))
        }
        return try (0..<batch).map { index in
            var budget = 0.0
            try words.withUnsafeBufferPointer { all in
                try heAmdCheck(he_bfv_noise_budget_from_norm(context.gpu, 64, level, all.baseAddress.map { $0 + index * limbs },
                                                             variableTime ? 1 : 0, &budget))
            }
            return budget
        }
    }

    /// `isTransparentCoeff` / `isTransparentEval` of `batch` resident ciphertexts: `flags` receives one byte each, 1 where
    /// every polynomial but the first is zero.  Enqueue-only.
    public static func gpuIsTransparent(resident ciphertexts: DeviceBuffer, batch: Int, polyCount: Int,
                                        polyContext: PolyContext<UInt64>, into flags: UnsafeMutablePointer<UInt8>,
                                        context: Context, on stream: HeAmdStream) throws
    {
        try heAmdCheck(he_bfv_is_transparent_device(context.gpu, 64, UInt32(polyContext.moduli.count), UInt32(polyCount),
                                                    ciphertexts.pointer, flags, batch, stream.raw))
    }
}
